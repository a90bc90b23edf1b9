"""hfv_frame_locate (the frame parser shared by the host helper and the extract kernel,
csrc/hfv_frame_parse.h) on the CPU: against a Python restatement of the reference parser
(br/src/bpf/parser.h:45-204, written from the reference text), against the router oracle's parse
verdicts, on the known PTF / IPv4-options / long-path frames, and over every truncation of a
valid frame.  Integer work: every comparison is exact."""
import struct

import numpy as np
import pytest

import br_fuzz as F
import br_topo as T
import orc
import scion_hfv as hfv
from scion_hfv import packets as P

V = hfv.VERDICT
MAC = lambda k, m: orc.cmac(m, k)   # noqa: E731  checker-side AES for building test paths
OK, PARSE_ERROR, NOT_SCION, NOT_IMPLEMENTED = 0, 17, 26, 34
BRS = ("br1", "br2", "br3")


def ref_parse(f: bytes, end: int):
    """parse_underlay + parse_scion + parse_scion_path over f[:end] (data_end = data + end):
    (status, inf_off, hf_off, checked) -- `checked` lists the offsets `data` was compared with
    data_end at, in order (the only places where a shorter frame can change the outcome)."""
    checked = []

    def beyond(x):
        checked.append(x)
        return x > end

    data = 14                                            # struct ethhdr
    if beyond(data):
        return NOT_SCION, 0, 0, checked
    h_proto = struct.unpack_from(">H", f, 12)[0]
    if h_proto == 0x0800:                                # ETH_P_IP
        ip = data
        data += 20                                       # struct iphdr
        if beyond(data):
            return NOT_SCION, 0, 0, checked
        skip = (4 * (f[ip] & 0x0F) - 20) % (1 << 64)     # size_t
        if skip > 40:
            return NOT_SCION, 0, 0, checked
        data += skip
        if f[ip + 9] != 17:                              # protocol != IPPROTO_UDP
            return NOT_SCION, 0, 0, checked
    elif h_proto == 0x86DD:                              # ETH_P_IPV6
        ip = data
        data += 40                                       # struct ipv6hdr
        if beyond(data):
            return NOT_SCION, 0, 0, checked
        if f[ip + 6] != 17:                              # nexthdr
            return NOT_SCION, 0, 0, checked
    else:
        return NOT_SCION, 0, 0, checked
    data += 8                                            # struct udphdr
    if beyond(data):
        return NOT_SCION, 0, 0, checked
    sc = data
    data += 28                                           # struct scionhdr: common header, dst and src ISD-AS
    if beyond(data):
        return PARSE_ERROR, 0, 0, checked
    if struct.unpack_from(">I", f, sc)[0] >> 28 != 0:    # SC_GET_VER
        return NOT_IMPLEMENTED, 0, 0, checked
    data += P.ref_host_addr_len(f[sc + 9])               # SC_GET_DL / SC_GET_SL (scion.h:50,52)
    if beyond(data):
        return PARSE_ERROR, 0, 0, checked
    if f[sc + 8] != 1:                                   # SC_PATH_TYPE_SCION
        return NOT_IMPLEMENTED, 0, 0, checked
    meta = data
    data += 4
    if beyond(data):
        return PARSE_ERROR, 0, 0, checked
    h = struct.unpack_from(">I", f, meta)[0]
    seg0, seg1, seg2 = (h >> 12) & 0x3F, (h >> 6) & 0x3F, h & 0x3F
    num_inf = (seg0 > 0) + (seg1 > 0) + (seg2 > 0)
    curr_inf, curr_hf = (h >> 30) & 0x03, (h >> 24) & 0x3F
    inf = data + 8 * curr_inf
    if beyond(inf + 8):
        return PARSE_ERROR, 0, 0, checked
    if curr_inf + 1 < num_inf and beyond(inf + 16):
        return PARSE_ERROR, 0, 0, checked
    hf = data + 8 * num_inf + 12 * curr_hf
    if beyond(hf + 12):
        return PARSE_ERROR, 0, 0, checked
    return OK, inf, hf, checked


def locate(frame_row, ln):
    """hfv_frame_locate as the kernel sees a slot: the whole slot in memory, `ln` bytes present."""
    buf = bytes(frame_row)
    inf, hf = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    st = hfv.lib().hfv_frame_locate(buf, int(ln), inf.ctypes.data_as(hfv.ctypes.POINTER(hfv.ctypes.c_uint32)),
                                    hf.ctypes.data_as(hfv.ctypes.POINTER(hfv.ctypes.c_uint32)))
    return st, int(inf[0]), int(hf[0])


_BATCHES = {}


def batch(br, v6):
    """The fuzz batch of the issue for (br, family), the parser's results on it, the restatement's
    results and the router oracle's verdicts; computed once and left unchanged."""
    if (br, v6) not in _BATCHES:
        brs = {b: T.OracleBR(T.br_config(b, v6)) for b in BRS}
        hops = F.hop_inputs(brs, v6, MAC)
        frames, lens, ifidx = F.fuzz_batch(hops, br, v6, 4096, seed=100 + v6, payload_max=1500)
        got = [locate(frames[i], lens[i]) for i in range(len(frames))]
        ref = [ref_parse(bytes(frames[i]), int(lens[i]))[:3] for i in range(len(frames))]
        _, verdict, _, _ = orc.br_process(frames.copy(), lens, ifidx, T.br_config(br, v6), orc.hop_key(T.KEYS[1]))
        for a in (frames, lens, ifidx, verdict):
            a.setflags(write=False)
        _BATCHES[(br, v6)] = (frames, lens, ifidx, got, ref, verdict)
    return _BATCHES[(br, v6)]


CASES = [(br, v6) for br in BRS for v6 in (False, True)]
IDS = [f"{br}-{'ipv6' if v6 else 'ipv4'}" for br, v6 in CASES]


@pytest.mark.parametrize("br,v6", CASES, ids=IDS)
def test_fuzz_parity_with_the_restatement(br, v6):
    _, _, _, got, ref, _ = batch(br, v6)
    bad = [(i, g, r) for i, (g, r) in enumerate(zip(got, ref)) if g != r]
    assert not bad, bad[:5]


@pytest.mark.parametrize("br,v6", CASES, ids=IDS)
def test_status_is_the_router_oracles_parse_verdict(br, v6):
    _, _, _, got, _, verdict = batch(br, v6)
    st = np.array([g[0] for g in got])
    failed = st != OK
    assert np.array_equal(verdict[failed], st[failed])
    assert (st[verdict == V["NOT_SCION"]] == NOT_SCION).all()


@pytest.mark.parametrize("br,v6", CASES, ids=IDS)
def test_fuzz_reaches_every_status(br, v6):
    _, _, _, got, _, _ = batch(br, v6)
    st = np.array([g[0] for g in got])
    counts = {s: int((st == s).sum()) for s in (OK, NOT_SCION, PARSE_ERROR, NOT_IMPLEMENTED)}
    print(br, v6, counts)
    assert counts[OK] >= 3000, counts
    for s in (NOT_SCION, PARSE_ERROR, NOT_IMPLEMENTED):
        assert counts[s] >= 100, counts
    assert sum(counts.values()) == len(st)


def _fields(frame, ln=None):
    st, inf, hf = hfv.frame_locate(frame) if ln is None else locate(frame, ln)
    return st, bytes(frame[inf:inf + 8]), bytes(frame[hf:hf + 12])


@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_ptf_frames_yield_the_paths_current_fields(v6):
    cases = F.ptf_cases(v6, MAC)
    assert len(cases) == 12
    k = 0
    for name, ing, egr in F.SCENARIOS:
        for kind in F.KINDS:
            path = P.ptf_path(kind, ing, egr, T.KEYS, seed=0x1234, mac_fn=MAC)
            frame = cases[k][2]
            k += 1
            st, inf, hf = _fields(frame)
            assert st == OK, (name, kind)
            assert inf == path.infos[path.curr_inf].pack(), (name, kind)
            assert hf == path.hops[path.curr_hf].pack(), (name, kind)


def test_ipv4_options_shift_the_offsets():
    brs = {b: T.OracleBR(T.br_config(b, False)) for b in BRS}
    frames, lens, _, m = F.options_shift_batch(F.hop_inputs(brs, False, MAC))
    assert m > 0 and len(frames) == 11 * m
    base = [locate(frames[j], lens[j]) for j in range(m)]
    for k in range(11):                                  # IHL 5 + k
        for j in range(m):
            st, inf, hf = locate(frames[k * m + j], lens[k * m + j])
            assert (st, inf, hf) == (OK, base[j][1] + 4 * k, base[j][2] + 4 * k), (k, j)
            assert frames[k * m + j, 14] == 0x40 | (5 + k)


@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_long_paths_hop_field_past_byte_256(v6):
    for k, (frame, _) in enumerate(F.long_path_frames(v6, MAC)):
        st, inf_off, hf_off = hfv.frame_locate(frame)
        assert st == OK and hf_off > 256
        # three segments, the current hop field is hop 3 + k of segment 1 (br_fuzz.long_path_frames)
        lens = [12 + k, 20, 10]
        path0 = 14 + (40 if v6 else 20) + 8 + 28 + 8
        assert inf_off == path0 + 4 + 8
        assert hf_off == path0 + 4 + 3 * 8 + 12 * (lens[0] + 3 + k)
        assert frame[inf_off] & 1 == 1                   # segment 1 is the Cons segment
        assert frame[hf_off + 2:hf_off + 6] == struct.pack(">HH", 1, 2)


@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
@pytest.mark.parametrize("kind", ["down", "seg_switch"])
def test_truncation(kind, v6):
    """len = 0 .. full length with the bytes left in place past len: OK only from the end of the
    current hop field on (seg_switch enters at the first info field of two, so the next info
    field is checked as well; it ends before the hop field does), and the status changes only at
    offsets the restatement compares with data_end."""
    ing_enc, _, _, _ = T.encaps(1, 2, v6)
    path = P.ptf_path(kind, 1, 2, T.KEYS, seed=5, mac_fn=MAC)
    frame = ing_enc.frame(P.scion_header(path.pack()))
    st_full, inf, hf, checked = ref_parse(frame, len(frame))
    assert st_full == OK
    first_ok = max(checked)
    assert first_ok == hf + 12
    if kind == "seg_switch":
        assert path.curr_inf == 0 and inf + 16 in checked
    prev = None
    for ln in range(len(frame) + 1):
        got = locate(frame, ln)
        want = ref_parse(frame, ln)[:3]
        assert got == want, ln
        assert (got[0] == OK) == (ln >= first_ok), ln
        if prev is not None and got[0] != prev:
            assert ln in checked, ln                     # a bound the parser checks, just reached
        prev = got[0]


@pytest.mark.skipif(not orc.ref_br_available(), reason="reference router not built (oracle/_ref)")
def test_status_is_the_reference_programs_parse_verdict():
    """The same claim held against the reference's own router program (br/src/bpf/xdp.c built as
    host code, orc.ref_br_process): on the mutation batches above and on every truncation of the
    frames of test_truncation, a non-zero status is the verdict that program records."""
    hk = orc.hop_key(T.KEYS[1])
    for br, v6 in CASES:
        frames, lens, ifidx, got, _, _ = batch(br, v6)
        verdict = orc.ref_br_process(frames.copy(), lens, ifidx, T.br_config(br, v6), hk)[1]
        st = np.array([g[0] for g in got])
        assert np.array_equal(verdict[st != OK], st[st != OK]), (br, v6)
        assert (st[verdict == V["NOT_SCION"]] == NOT_SCION).all()
    for v6 in (False, True):
        for kind in ("down", "seg_switch"):
            ing_enc, _, _, ifi = T.encaps(1, 2, v6)
            frame = ing_enc.frame(P.scion_header(P.ptf_path(kind, 1, 2, T.KEYS, seed=5, mac_fn=MAC).pack()))
            rows, _ = T.to_slots([frame] * (len(frame) + 1), slot=256)
            lens = np.arange(len(frame) + 1, dtype=np.uint16)
            st = np.array([locate(frame, ln)[0] for ln in lens])
            verdict = orc.ref_br_process(rows, lens, np.full(len(lens), ifi, np.uint32), T.br_config("br1", v6), hk)[1]
            assert np.array_equal(verdict[st != OK], st[st != OK]), (kind, v6)
            assert (st != OK).sum() >= 100 and verdict[-1] == V["SCION_FORWARD"]


def test_frame_locate_arguments():
    L = hfv.lib()
    u = hfv.ctypes.c_uint32()
    assert L.hfv_frame_locate(None, 64, hfv.ctypes.byref(u), hfv.ctypes.byref(u)) == -hfv.errno.EINVAL
    assert L.hfv_frame_locate(b"\0" * 64, 64, None, hfv.ctypes.byref(u)) == -hfv.errno.EINVAL
    assert hfv.frame_locate(b"") == (NOT_SCION, 0, 0)
    assert (hfv.FRAME_OK, hfv.FRAME_PARSE_ERROR, hfv.FRAME_NOT_SCION, hfv.FRAME_NOT_IMPLEMENTED) == (
        OK, V["PARSE_ERROR"], V["NOT_SCION"], V["NOT_IMPLEMENTED"])
    assert hfv.FRAME_REC_STRIDE == 24
