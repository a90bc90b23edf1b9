"""hfv_frame_extract (csrc/hfv_frames_host.cpp) on the CPU: the host counterpart of the
direction-aware extract kernel.  Against the two MAC-chaining rules of the reference restated in
Python (frames_rx_ref.beta_ingress / beta_egress, from path_processing.h:72-81 and 138-148),
against hfv_frame_locate plus a gather, against the router oracle's verdicts over the normalised
records, and over every truncation of one internal frame.  Integer work: every comparison is exact.
"""
import ctypes
import errno

import numpy as np
import pytest

import br_topo as T
import frames_rx_ref as R
import orc
import scion_hfv as hfv

V = hfv.VERDICT


@pytest.mark.parametrize("internal", [0, 1], ids=["external", "internal"])
@pytest.mark.parametrize("br,v6", R.CASES, ids=R.IDS)
def test_frame_extract_applies_the_rule_of_the_direction(br, v6, internal):
    """The verify kernels compute beta by the ingress rule from the record.  For an external frame
    that must be the ingress rule's beta of the frame, for an internal one the egress rule's; the
    status is hfv_frame_locate's, and no byte but the SegID differs from the frame's fields."""
    b = R.batch(br, v6)
    st, inf, hf = R.frame_extract(b.frames, b.lens, bool(internal))
    assert np.array_equal(st, b.status)
    ok = np.nonzero(st == 0)[0]
    assert len(ok) >= 3000
    assert not inf[st != 0].any() and not hf[st != 0].any()
    assert np.array_equal(hf, b.hf)
    assert np.array_equal(inf[:, [0, 1, 4, 5, 6, 7]], b.inf[:, [0, 1, 4, 5, 6, 7]])
    rule = R.beta_egress if internal else R.beta_ingress
    changed = 0
    for i in ok:
        want = rule(bytes(b.inf[i]), bytes(b.hf[i]))
        assert R.beta_ingress(bytes(inf[i]), bytes(hf[i])) == want, i
        changed += bytes(inf[i]) != bytes(b.inf[i])
    if internal:
        folds = ~b.cons[ok] & (b.hf[ok, 6:8] != 0).any(axis=1)          # a MAC[0:2] of 0 changes nothing
        assert folds.sum() >= 1000 and changed == folds.sum()
    else:
        assert changed == 0 and np.array_equal(inf, b.inf)              # hfv_frame_locate + a gather


@pytest.mark.parametrize("br,v6", R.CASES, ids=R.IDS)
def test_normalised_records_vs_router_oracle(br, v6):
    """Records by hfv_frame_extract with the batch's own directions, verified by the record oracle:
    on the frames decided by the MAC the bit is the router oracle's SCION_FORWARD."""
    b = R.batch(br, v6)
    R.check_selection_counts(b, br)
    hk, valid = orc.key_table(T.KEYS[1])
    st, inf, hf = R.frame_extract(b.frames, b.lens, b.internal)
    bits = hfv.bits_to_bool(R.oracle_bits(st, inf, hf, hk, valid, hfv.KEYSEL_ZERO), 4096)
    assert (st[b.sel] == 0).all()
    assert np.array_equal(bits[b.sel], b.forward[b.sel])
    # without the normalisation (every frame taken as external) the ingress rule misjudges the
    # internal link's frames
    plain = hfv.bits_to_bool(R.oracle_bits(b.status, b.inf, b.hf, hk, valid, hfv.KEYSEL_ZERO), 4096)
    assert np.array_equal(plain[b.sel_ext], b.forward[b.sel_ext])
    wrong = int((plain[b.sel_int] != b.forward[b.sel_int]).sum())
    print(br, v6, "internal selected", int(b.sel_int.sum()), "ingress rule wrong on", wrong)
    if br in ("br2", "br3"):
        assert wrong >= 500, wrong


def known_internal_frame():
    """The first frame of the br2 IPv4 batch that came over the internal link with a Cons = 0
    InfoField and was forwarded."""
    b = R.batch("br2", False)
    i = int(np.nonzero(b.sel_int & ~b.cons & b.forward)[0][0])
    return bytes(b.frames[i]), int(b.lens[i])


def test_truncation_of_an_internal_frame():
    frame, full = known_internal_frame()
    L = hfv.lib()
    a, c = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.hfv_frame_locate(frame, full, ctypes.byref(a), ctypes.byref(c)) == 0
    st, inf0, hf0 = hfv.frame_extract(frame[:full], True)
    assert st == 0 and hf0 == frame[c.value:c.value + 12]
    assert inf0[2:4] == bytes(x ^ y for x, y in zip(frame[a.value + 2:a.value + 4], hf0[6:8]))
    assert inf0[2:4] != frame[a.value + 2:a.value + 4]
    seen = set()
    for ln in range(full + 1):
        inf, hf = ctypes.create_string_buffer(b"\xEE" * 8, 8), ctypes.create_string_buffer(b"\xEE" * 12, 12)
        got = L.hfv_frame_extract(frame, ln, 1, inf, hf)
        assert got == L.hfv_frame_locate(frame, ln, ctypes.byref(a), ctypes.byref(c)), ln
        seen.add(got)
        if got != 0:
            assert inf.raw == bytes(8) and hf.raw == bytes(12), ln
        else:
            assert (inf.raw, hf.raw) == (inf0, hf0), ln
    assert seen == {0, 17, 26}


def test_frame_extract_arguments():
    L = hfv.lib()
    frame, full = known_internal_frame()
    inf, hf = ctypes.create_string_buffer(8), ctypes.create_string_buffer(12)
    E = -errno.EINVAL
    assert L.hfv_frame_extract(None, 64, 0, inf, hf) == E
    assert L.hfv_frame_extract(frame, full, 0, None, hf) == E
    assert L.hfv_frame_extract(frame, full, 1, inf, None) == E
    assert L.hfv_ctx_set_internal_ifindices(None, None, 0) == E
    assert hfv.frame_extract(b"", True) == (hfv.FRAME_NOT_SCION, bytes(8), bytes(12))
    st, a, b = hfv.frame_extract(frame[:full])
    assert (st, a, b) == hfv.frame_extract(frame[:full], False) and st == 0
