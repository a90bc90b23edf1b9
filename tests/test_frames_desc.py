"""hfv_verify_frames_desc without a GPU: the entry points are declared, exported by the product and
the test library and wrapped in Python; struct hfv_frame_desc is 16 bytes with its fields at 0, 8 and
12, as FrameDesc and FRAME_DESC_DTYPE are; the ABI version stays 3; a NULL ctx or a NULL kernel_ms is
-EINVAL before any device work (the checks that need a ctx are in test_gpu_frames_desc.py);
hfv_frame_desc_ok agrees with the rule restated on Python integers at every boundary; the corpora of
tests/frames_desc.py exercise what their placement tables say; and the host judge gives the same
verdicts whether it reads a frame where the descriptor points or from the slot copy."""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import br_shift as S
import br_topo as T
import frames_desc as D
import frames_rx_ref as R
import orc
import scion_hfv as hfv

NAMES = ("hfv_verify_frames_desc", "hfv_verify_frames_desc_timed", "hfv_frame_desc_ok")
K1 = T.KEYS[1]


# ---- the host judge -----------------------------------------------------------------------------

def host_judge(buf, umem_off, umem_bytes, desc, iset, hop_keys, valid_keys, keysel):
    """(bitmap words, status) by hfv_frame_extract on the bytes each valid descriptor names, where
    they lie in the UMEM, and the record checker (the oracle() of test_gpu_frames_fused.py, fed from
    the buffer instead of from slots).  An invalid descriptor: status 255, bit 0; nothing is read for
    it."""
    n = len(desc)
    buf = np.ascontiguousarray(buf)
    L = hfv.lib()
    status = np.zeros(n, dtype=np.uint8)
    inf = np.full((n, 8), 0xEE, dtype=np.uint8)
    hf = np.full((n, 12), 0xEE, dtype=np.uint8)
    base = buf.ctypes.data + umem_off
    internal = np.isin(desc["ifindex"], iset) if len(iset) else np.zeros(n, dtype=bool)
    for i in range(n):
        a, w = int(desc["addr"][i]), int(desc["len"][i])
        if not D.desc_ok(a, w, umem_bytes):
            status[i] = D.BAD_DESC
            continue
        rc = L.hfv_frame_extract(base + a, w, int(internal[i]), inf[i].ctypes.data, hf[i].ctypes.data)
        assert rc >= 0
        status[i] = rc
    return R.oracle_bits(status, inf, hf, hop_keys, valid_keys, keysel), status


def slot_judge(frames, lens, ifidx, iset, hop_keys, valid_keys, keysel, valid=None):
    """The same judge on a slot copy: the oracle() of test_gpu_frames_fused.py; rows of invalid
    descriptors (valid[i] false) get status 255 and bit 0."""
    n = len(frames)
    internal = np.isin(ifidx, iset) if len(iset) else np.zeros(n, dtype=bool)
    st, inf, hf = R.frame_extract(np.ascontiguousarray(frames), lens, internal)
    if valid is not None:
        st[~valid] = D.BAD_DESC
    return R.oracle_bits(st, inf, hf, hop_keys, valid_keys, keysel), st


_KEYS = {}


def key1():
    if "k1" not in _KEYS:
        _KEYS["k1"] = orc.key_table(K1)
    return _KEYS["k1"]


# ---- declarations, exports, wrappers ------------------------------------------------------------

def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_entry_points_declared_and_exported():
    src = open(os.path.join(orc.ROOT, "include", "scion_hfv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), name
    assert re.search(r"#define\s+HFV_ABI_VERSION\s+3\b", src)
    assert re.search(r"#define\s+HFV_FRAME_DESC_MAX_LEN\s+65535u\b", src)
    assert re.search(r"#define\s+HFV_FRAME_BAD_DESC\s+255\b", src)
    assert re.search(r"struct\s+hfv_frame_desc\s*\{\s*uint64_t\s+addr;\s*uint32_t\s+len;\s*uint32_t\s+ifindex;\s*\}", src)
    for path in (hfv.LIB_PATH, hfv.TEST_LIB_PATH):
        assert set(NAMES) <= _exports(path), path
    assert hfv.lib().hfv_abi_version() == 3


def test_python_wrappers_and_descriptor_layout():
    for name in ("verify_frames_desc", "verify_frames_desc_timed"):
        sig = inspect.signature(getattr(hfv.Ctx, name))
        assert list(sig.parameters) == ["self", "umem", "umem_bytes", "desc", "n", "pass_bits", "status", "stream"]
        assert all(sig.parameters[p].default is None for p in ("status", "stream"))
    assert list(inspect.signature(hfv.frame_desc_ok).parameters) == ["addr", "len", "umem_bytes"]
    assert ctypes.sizeof(hfv.FrameDesc) == 16
    assert [(f, getattr(hfv.FrameDesc, f).offset) for f in ("addr", "len", "ifindex")] == [("addr", 0), ("len", 8),
                                                                                          ("ifindex", 12)]
    dt = hfv.FRAME_DESC_DTYPE
    assert dt.itemsize == 16 and dt.names == ("addr", "len", "ifindex")
    assert [dt.fields[f][1] for f in dt.names] == [0, 8, 12]
    assert [dt.fields[f][0] for f in dt.names] == [np.dtype("<u8"), np.dtype("<u4"), np.dtype("<u4")]
    assert dt == D.DTYPE
    one = np.zeros(1, dtype=dt)
    one[0] = (0x1122334455667788, 0xA1B2C3D4, 0x0BADF00D)
    c = hfv.FrameDesc.from_buffer_copy(one.tobytes())
    assert (c.addr, c.len, c.ifindex) == (0x1122334455667788, 0xA1B2C3D4, 0x0BADF00D)
    assert (hfv.FRAME_BAD_DESC, hfv.FRAME_DESC_MAX_LEN) == (255, 65535) == (D.BAD_DESC, D.MAX_LEN)
    assert hfv.FRAME_BAD_DESC not in hfv.VERDICT.values()


def test_rejects_bad_arguments_without_gpu():
    """A NULL ctx, and a NULL kernel_ms in the timed form, fail with -EINVAL before any device work,
    whatever the other arguments are."""
    L = hfv.lib()
    E = -errno.EINVAL
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    ms = ctypes.c_float(-1.0)
    assert L.hfv_verify_frames_desc(None, p, 256, p, 1, None, p, None) == E
    assert "NULL" in L.hfv_last_error().decode()
    assert L.hfv_verify_frames_desc(None, None, 0, None, 0, None, None, None) == E               # even with n == 0
    assert L.hfv_verify_frames_desc_timed(None, p, 256, p, 1, None, p, None, ctypes.byref(ms)) == E
    assert L.hfv_verify_frames_desc_timed(None, p, 256, p, 1, None, p, None, None) == E
    assert "null" in L.hfv_last_error().decode()
    assert ms.value == -1.0                                   # nothing written on the failed call
    assert bytes(buf) == bytes(256)


# ---- the validity rule --------------------------------------------------------------------------

UMEMS = (0, 1, 15, 16, 64, 4096, 65534, 65535, 65536, 65537, 1 << 20, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, 1 << 40,
         (1 << 63) - 1, 1 << 63, (1 << 64) - 9, (1 << 64) - 8, (1 << 64) - 1)
LENS = (0, 1, 8, 65535, 65536, (1 << 32) - 1)
M64 = (1 << 64) - 1


def test_frame_desc_ok_boundaries():
    ok = yes = 0
    for ub in UMEMS:
        for addr in (0, (ub - 1) & M64, ub, (ub + 1) & M64, 1 << 63, (1 << 64) - 8, M64):
            for ln in LENS:
                want = D.desc_ok(addr, ln, ub)
                assert hfv.frame_desc_ok(addr, ln, ub) is want, (addr, ln, ub)
                ok += 1
                yes += want
    assert ok == len(UMEMS) * 7 * len(LENS) and 100 < yes < ok - 100
    # what a wrapping sum would get wrong
    assert not hfv.frame_desc_ok((1 << 64) - 8, 16, 1 << 20)
    assert not hfv.frame_desc_ok((1 << 64) - 1, 1, M64 - 1)
    assert hfv.frame_desc_ok(M64, 0, M64) and not hfv.frame_desc_ok(M64, 1, M64)
    assert hfv.frame_desc_ok(4096, 0, 4096) and not hfv.frame_desc_ok(4097, 0, 4096)


def test_frame_desc_ok_random_pairs():
    rng = np.random.default_rng(20260)
    yes = 0
    for _ in range(10000):
        ub = int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
        addr = int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
        if rng.random() < 0.5:                               # near the end of the buffer
            addr = max(0, ub - int(rng.integers(0, 70000)))
        ln = int(rng.integers(0, 1 << 32)) >> int(rng.integers(0, 32))
        want = D.desc_ok(addr, ln, ub)
        assert hfv.frame_desc_ok(addr, ln, ub) is want, (addr, ln, ub)
        yes += want
    assert 2000 < yes < 8000


# ---- the corpora --------------------------------------------------------------------------------

# packed layouts: (frames, frames per addr & 15, frames at addr 0 -- the first, and any of length 0
# in front of it).  br_shift's corpus frames have even lengths, so they reach the even residues only;
# the fuzz batches and the truncation sweeps reach all sixteen.
PACKED = {
    "fuzz_br1_0": (4096, (240, 240, 281, 255, 257, 256, 264, 284, 230, 271, 261, 264, 238, 234, 264, 257), 1),
    "fuzz_br1_1": (4096, (269, 259, 268, 285, 217, 249, 251, 235, 254, 272, 235, 239, 262, 297, 258, 246), 1),
    "fuzz_br2_0": (4096, (237, 247, 233, 270, 270, 241, 280, 268, 262, 246, 257, 265, 256, 242, 270, 252), 1),
    "fuzz_br2_1": (4096, (273, 259, 248, 242, 278, 246, 264, 282, 280, 238, 234, 269, 206, 261, 275, 241), 1),
    "fuzz_br3_0": (4096, (251, 246, 267, 284, 257, 274, 243, 257, 232, 280, 246, 252, 231, 267, 270, 239), 1),
    "fuzz_br3_1": (4096, (273, 264, 244, 251, 253, 252, 246, 285, 227, 276, 248, 237, 264, 281, 253, 242), 1),
    "corpus_0_br1": (1188, (149, 0, 150, 0, 154, 0, 150, 0, 148, 0, 147, 0, 143, 0, 147, 0), 1),
    "corpus_0_br2": (792, (99, 0, 99, 0, 99, 0, 99, 0, 99, 0, 99, 0, 99, 0, 99, 0), 1),
    "corpus_0_br3": (396, (50, 0, 51, 0, 55, 0, 51, 0, 49, 0, 48, 0, 44, 0, 48, 0), 1),
    "corpus_1_br1": (108, (14, 0, 12, 0, 13, 0, 12, 0, 13, 0, 15, 0, 14, 0, 15, 0), 1),
    "corpus_1_br2": (72, (9, 0, 9, 0, 9, 0, 9, 0, 9, 0, 9, 0, 9, 0, 9, 0), 1),
    "corpus_1_br3": (36, (5, 0, 3, 0, 4, 0, 3, 0, 4, 0, 6, 0, 5, 0, 6, 0), 1),
    "sweep_0": (4755, (301, 294, 297, 301, 294, 296, 302, 295, 295, 301, 297, 294, 300, 298, 292, 298), 2),
    "sweep_1": (2697, (171, 170, 170, 170, 170, 169, 169, 169, 168, 168, 167, 166, 166, 167, 168, 169), 2),
}
EDGES = {   # umem_bytes, placement() of frames_desc.edge_cases(*edge_source())
    "tail_0_60": (6268, (9, (2, 0, 1, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 1, 1, 1), 1, 1, 0, 0, 0)),
    "tail_1_127": (6336, (9, (1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 1, 1, 1), 1, 1, 0, 0, 0)),
    "tail_7_100": (6299, (9, (1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 2, 0, 0, 1, 1, 1), 1, 1, 0, 0, 0)),
    "tail_8_64": (6264, (9, (1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 1, 1), 1, 1, 0, 0, 0)),
    "tail_15_77": (6284, (9, (1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 1, 1, 2), 1, 1, 0, 0, 0)),
    "odd": (6413, (9, (1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 2, 0, 0, 1, 1, 1), 0, 1, 0, 0, 0)),
    "one64": (64, (1, (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), 1, 1, 0, 0, 0)),
}
REPEATS = (68, (66, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), 0, 66, 63, 68, 0)


def test_placement_tables():
    assert {s for s, _ in D.CORPORA} == set(PACKED) and len(D.CORPORA) == 3 * len(PACKED)
    for src, kind in D.CORPORA + D.SHIFTED:
        buf, off, nbytes, desc = D.corpus(src, kind)
        assert off == D.GUARD and len(buf) == nbytes + 2 * D.GUARD
        n, mod16, a0 = PACKED[src]
        if kind == "packed":
            want = (n, mod16, 0, a0, 0, 0, 0)
        else:   # one frame per 2048-byte chunk at headroom 256 (+ k): nothing at 0, nothing near the end
            k = kind[1] if isinstance(kind, tuple) else 0
            want = (n, tuple(n if r == k else 0 for r in range(16)), 0, 0, 0, 0, 0)
            assert nbytes == n * D.CHUNK and sorted(desc["addr"] // D.CHUNK) == list(range(n))
            assert ((desc["addr"] % D.CHUNK) == D.HEADROOM + k).all()
        assert D.placement(desc, nbytes) == want, (src, kind)
    for src in D.FUZZ + ("sweep_0", "sweep_1"):
        assert min(PACKED[src][1]) > 0, src                  # every addr & 15
    order = D.corpus("fuzz_br1_0", "permuted")[3]["addr"]
    assert (np.diff(order.astype(np.int64)) < 0).sum() > 1000   # really out of order
    cases = D.edge_cases(*D.edge_source())
    assert [c[0] for c in cases] == list(EDGES)
    for name, buf, off, nbytes, desc in cases:
        assert (nbytes, D.placement(desc, nbytes)) == EDGES[name], name
        if name.startswith("tail"):
            k, cut = (int(x) for x in name.split("_")[1:])
            a, w = int(desc["addr"][-1]), int(desc["len"][-1])
            assert a % 16 == k and w == cut < D.WIN and a + w == nbytes and desc["addr"][0] == 0
    assert EDGES["odd"][0] % 2 == 1
    f, l, i = D.edge_source()
    c = D.repeat_case(f, l, i, 99)
    assert D.placement(c[3], c[2]) == REPEATS


def test_layout_round_trip_and_guards():
    """slot_copy of a layout gives the frames back; filler reaches every byte no frame covers; a
    spilled tail leaves the whole frame behind the cut one."""
    frames, lens, ifidx = D.edge_source()
    pat = bytes(range(1, 200))
    for kind in D.KINDS + (("shift", 5), "odd", ("tail", 7, 100)):
        buf, off, nbytes, desc = D.layout(frames, lens, kind, seed=3, filler=pat, ifindex=ifidx)
        got, gl, gi, valid = D.slot_copy(buf, off, nbytes, desc, slot=frames.shape[1])
        assert valid.all() and np.array_equal(gi, ifidx)
        assert np.array_equal(gl, desc["len"]) and (gl[:-1] == lens[:-1]).all()
        covered = np.zeros(len(buf), dtype=bool)
        for i in range(len(desc)):
            assert np.array_equal(got[i, :gl[i]], frames[i, :gl[i]])
            a = off + int(desc["addr"][i])
            covered[a:a + gl[i]] = True
        assert np.array_equal(buf[~covered], D.fill(len(buf), pat)[~covered])
        assert not covered[:off].any() and not covered[off + nbytes:].any()
    buf, off, nbytes, desc = D.layout(frames, lens, ("tail", 7, 100), filler=0xFF, ifindex=ifidx, spill=True)
    a = off + int(desc["addr"][-1])
    assert np.array_equal(buf[a:a + lens[-1]], frames[-1, :lens[-1]]) and a + 100 == off + nbytes
    with pytest.raises(AssertionError):
        D.plant(buf, off, nbytes + D.GUARD, b"\x00" * 8)


CORPUS_IDS = ["%s-%s" % (s, D.kind_name(k)) for s, k in D.CORPORA]


@pytest.mark.parametrize("src,kind", D.CORPORA, ids=CORPUS_IDS)
def test_host_judge_is_independent_of_layout(src, kind):
    """hfv_frame_extract on the bytes where the descriptor points, against the same judge on the
    slots the corpus was laid out from, with the BR's internal interfaces as the set."""
    frames, lens, ifidx, _, _ = D.source(src)
    iset = D.internal_set(src)
    buf, off, nbytes, desc = D.corpus(src, kind)
    hk, vk = key1()
    got, got_st = host_judge(buf, off, nbytes, desc, iset, hk, vk, hfv.KEYSEL_ZERO)
    want, want_st = slot_judge(frames, lens, ifidx, iset, hk, vk, hfv.KEYSEL_ZERO)
    assert np.array_equal(got_st, want_st) and np.array_equal(got, want)
    assert (want_st == 0).sum() >= len(frames) // 8 and want.any()      # (the sweeps are mostly cut frames)
    if src.startswith("fuzz"):
        for s in (0, 17, 26, 34):
            assert (want_st == s).any(), s


def test_host_judge_on_edges_and_bad_descriptors():
    """The cut tail frame fails (its header is cut) although the whole frame passes; invalid
    descriptors get status 255 and bit 0 and are never followed."""
    frames, lens, ifidx = D.edge_source()
    hk, vk = key1()
    full, _ = slot_judge(frames, lens, ifidx, [], hk, vk, hfv.KEYSEL_ZERO)
    assert int(full[0]) == (1 << len(frames)) - 1            # every edge frame passes when whole
    hdr = S.header_end(bytes(frames[-1, :lens[-1]]))         # the cut frame's headers end here
    cut_short = 0
    for name, buf, off, nbytes, desc in D.edge_cases(frames, lens, ifidx, filler=0xFF, spill=True):
        got, st = host_judge(buf, off, nbytes, desc, [], hk, vk, hfv.KEYSEL_ZERO)
        f, l, i, valid = D.slot_copy(buf, off, nbytes, desc)
        want, want_st = slot_judge(f, l, i, [], hk, vk, hfv.KEYSEL_ZERO, valid)
        assert np.array_equal(got, want) and np.array_equal(st, want_st), name
        if name.startswith("tail") or name == "one64":             # cut inside the header: no verdict but 0
            whole = int(desc["len"][-1]) >= hdr
            assert (st[-1] == 0) == whole and (int(got[0]) >> (len(desc) - 1)) & 1 == whole, name
            cut_short += not whole
    assert cut_short >= 4
    buf, off, nbytes, desc = D.layout(frames, lens, "packed", ifindex=ifidx)
    desc = desc.copy()
    desc["addr"][2] = nbytes + 1
    desc["addr"][4], desc["len"][4] = nbytes - 8, 16
    desc["len"][5] = 65536
    desc["addr"][7], desc["len"][7] = (1 << 64) - 8, 16
    got, st = host_judge(buf, off, nbytes, desc, [], hk, vk, hfv.KEYSEL_ZERO)
    bad = np.array([2, 4, 5, 7])
    assert (st[bad] == 255).all() and (np.delete(st, bad) == 0).all()
    assert int(got[0]) == ((1 << len(desc)) - 1) & ~sum(1 << int(b) for b in bad)
