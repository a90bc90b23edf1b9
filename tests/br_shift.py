"""Forwardable frames whose SCION path sits on every edge of the 128-byte staging window.

The router kernel (hfv_br_kernel.hip) and the extract kernel (hfv_frames_kernel.hip) read the
first 128 bytes of a frame from LDS, bytes 128-135 from registers (the router, for frames
whose HdrLen says the header runs that far) and the rest from HBM; which case a header field
takes depends only on where the parse places it.  The frames of packets.py carry 4-byte host
addresses, so their PathMeta sits at byte 78 (IPv4) or 98 (IPv6), and IPv4 options alone move
it to 118 at most.  This module owns the corpus that moves the path further, and its rule:

  * the reference's parser skips 8 + 4*DL + 4*SL bytes of host addresses with
    DL = (haddr >> 2) & 2 and SL = (haddr >> 6) & 2 (include/bpf/scion.h:50,52, parser.h:133;
    packets.ref_host_addr_len), so haddr bit 0x08 and/or 0x80 plus 8 or 16 filler bytes after
    the two 4-byte host addresses move the whole path by 8 or 16 bytes
    (with_host_addr_fill);
  * 0..10 IPv4 option words move it by another 0..40 bytes (br_fuzz.with_ipv4_options).

The router never looks at host addresses, lengths or HdrLen and updates the checksums
incrementally without checking them, so every shifted frame is routed as its base is (checked on
the CPU in tests/test_br_shift.py, against the reference program where it is built).

field_offsets restates the parser's placement rule in plain Python integers, independent of
the C and HIP code.  Test infrastructure only.
"""
import hashlib
import struct

import numpy as np

import br_fuzz as F
import br_topo as T
import orc
from scion_hfv import packets as P

MAC = lambda k, m: orc.cmac(m, k)   # noqa: E731  checker-side AES for building test paths
BRS = ("br1", "br2", "br3")
SLOT = 256
EDGES = (128, 136)                 # end of the staged row, end of the router's ext registers
HADDR_BITS = (0x00, 0x08, 0x88)    # j = 0..2: DL bit 1, then DL and SL bit 1
FILL = bytes(0xA1 + 7 * i & 0xFF | 0x80 for i in range(16))   # non-zero, no two neighbours equal
V4_SHIFTS = tuple((k, j) for k in range(11) for j in range(3))
V6_SHIFTS = tuple((0, j) for j in range(3))
SWEEP_V4 = ((0, 0), (0, 10), (1, 10), (2, 8), (2, 10))   # (j, k)
SWEEP_V6 = (0, 1, 2)                                    # j
HOST_WINDOWS = (104, 112, 120, 128, 136, 144, 152, 160)
HOST_WINDOWS_ALL_ABOVE = (64, 88)


def scion_offset(frame: bytes, v6: bool) -> int:
    return 14 + (40 if v6 else 4 * (frame[14] & 15)) + 8


def with_host_addr_fill(frame: bytes, v6: bool, j: int) -> bytes:
    """The frame with haddr |= HADDR_BITS[j] and 8*j filler bytes after the source host address:
    the parser skips them as host-address bytes, so the path moves by 8*j.  For a frame without
    IPv4 options (apply with_ipv4_options afterwards).  Lengths and checksums are left stale on
    purpose: the router does not check them."""
    sc = scion_offset(frame, v6)
    g = bytearray(frame)
    g[sc + 9] |= HADDR_BITS[j]
    at = sc + 28 + 8
    return bytes(g[:at]) + FILL[:8 * j] + bytes(g[at:])


def shifted(frame: bytes, v6: bool, k: int, j: int) -> bytes:
    f = with_host_addr_fill(frame, v6, j)
    return f if v6 else F.with_ipv4_options(f, k)


def unshifted(frame: bytes, v6: bool, k: int, j: int) -> bytes:
    """A shifted frame (input or output) with the inserted bytes removed and the two changed
    header bytes (IHL, haddr) put back."""
    g = bytearray(frame)
    if not v6:
        g = g[:34] + g[34 + 4 * k:]
        g[14] = 0x45
    sc = scion_offset(g, v6)
    g = g[:sc + 36] + g[sc + 36 + 8 * j:]
    g[sc + 9] &= 0xFF ^ HADDR_BITS[j]
    return bytes(g)


_CACHE = {}


def hop_inputs(v6):
    """br_fuzz.hop_inputs with the default seeds: [(br, ingress ifindex, frame)], built once."""
    if ("hops", v6) not in _CACHE:
        brs = {b: T.OracleBR(T.br_config(b, v6)) for b in BRS}
        _CACHE[("hops", v6)] = F.hop_inputs(brs, v6, MAC)
    return _CACHE[("hops", v6)]


def shift_corpus(v6):
    """{br: (frames u8[n, 256], lens u16[n], ifindex u32[n], shift_id[n], base_id[n])}: every hop
    input of the BR at every shift, shift-major (shift_id indexes V4_SHIFTS / V6_SHIFTS, base_id
    the BR's hop inputs in the order of br_fuzz.hop_inputs).  Built once and left unchanged."""
    if ("corpus", v6) not in _CACHE:
        shifts = V6_SHIFTS if v6 else V4_SHIFTS
        out = {}
        for br in BRS:
            mine = [(i, f) for b, i, f in hop_inputs(v6) if b == br]
            fl, ifi, sid, bid = [], [], [], []
            for s, (k, j) in enumerate(shifts):
                for b, (i, f) in enumerate(mine):
                    fl.append(shifted(f, v6, k, j))
                    ifi.append(i), sid.append(s), bid.append(b)
            frames, lens = T.to_slots(fl, slot=SLOT)
            out[br] = (frames, lens, np.array(ifi, np.uint32), np.array(sid, np.int32), np.array(bid, np.int32))
            for a in out[br]:
                a.setflags(write=False)
        _CACHE[("corpus", v6)] = out
    return _CACHE[("corpus", v6)]


def field_offsets(frame: bytes):
    """{name: (offset, size)} of the header fields the kernels read past the fixed part, by the
    parser's own rule (parser.h:45-204) in plain integers: PathMeta, the current info field's
    SegID, the next info field's SegID (None unless curr_inf + 1 < num_inf), the current hop
    field and its MAC; plus "inf" and "hf", the two offsets themselves."""
    proto = struct.unpack_from(">H", frame, 12)[0]
    if proto == 0x0800:
        udp = 14 + 4 * (frame[14] & 0x0F)
    else:
        assert proto == 0x86DD
        udp = 14 + 40
    sc = udp + 8
    meta = sc + 28 + P.ref_host_addr_len(frame[sc + 9])
    h = struct.unpack_from(">I", frame, meta)[0]
    num_inf = sum(1 for sh in (12, 6, 0) if (h >> sh) & 0x3F)
    curr_inf, curr_hf = h >> 30, (h >> 24) & 0x3F
    inf = meta + 4 + 8 * curr_inf
    hf = meta + 4 + 8 * num_inf + 12 * curr_hf
    return {"meta": (meta, 4), "seg0": (inf + 2, 2), "seg1": (inf + 10, 2) if curr_inf + 1 < num_inf else None,
            "hf": (hf, 12), "mac": (hf + 6, 6), "inf_off": inf, "hf_off": hf}


FIELDS = ("meta", "seg0", "seg1", "hf", "mac")


def header_end(frame: bytes) -> int:
    """One past the last header byte the router uses: the end of the current hop field, or of the
    next info field where there is one, whichever is larger."""
    o = field_offsets(frame)
    end = o["hf"][0] + 12
    if o["seg1"] is not None:
        end = max(end, o["seg1"][0] - 2 + 8)
    return end


def corpus_frames(corpus):
    """The frames (bytes) of one shift_corpus()[br] entry, or of a list of them."""
    if isinstance(corpus, tuple):
        corpus = [corpus]
    return [bytes(c[0][i, :c[1][i]]) for c in corpus for i in range(len(c[0]))]


def placement_table(corpus, edges=EDGES):
    """{(field, edge): {"in": n, "straddle": {split: n}, "past": n}} over the frames of `corpus`
    (shift_corpus entries): a field lies in front of the edge, across it (split = bytes in
    front), or at and past it.  Frames without the field (seg1) are not counted."""
    table = {(f, e): {"in": 0, "straddle": {}, "past": 0} for f in FIELDS for e in edges}
    for frame in corpus_frames(corpus):
        o = field_offsets(frame)
        for f in FIELDS:
            if o[f] is None:
                continue
            off, size = o[f]
            for e in edges:
                cell = table[(f, e)]
                if off + size <= e:
                    cell["in"] += 1
                elif off >= e:
                    cell["past"] += 1
                else:
                    cell["straddle"][e - off] = cell["straddle"].get(e - off, 0) + 1
    return table


def sweep_bases(v6):
    """[(name, kind, frame, ifindex)]: the four path kinds of the br1 "direct" scenario and the
    "sibling" seg_switch frame."""
    return [(name, kind, frame, ifi) for name, kind, frame, _, ifi, _, _ in F.ptf_cases(v6, MAC)
            if name == "direct" or (name == "sibling" and kind == "seg_switch")]


def truncation_sweep(v6):
    """(frames u8[n, 256], lens u16[n], ifindex u32[n]) for br1: each sweep base at each sweep
    shift, once per length 0..full (the same bytes, only len varies).  Built once."""
    if ("sweep", v6) not in _CACHE:
        shifts = [(0, j) for j in SWEEP_V6] if v6 else [(k, j) for j, k in SWEEP_V4]
        rows, lens, ifi = [], [], []
        for _, _, frame, i in sweep_bases(v6):
            for k, j in shifts:
                f = shifted(frame, v6, k, j)
                row = np.zeros(SLOT, np.uint8)
                row[:len(f)] = np.frombuffer(f, np.uint8)
                rows += [row] * (len(f) + 1)
                lens += range(len(f) + 1)
                ifi += [i] * (len(f) + 1)
        out = (np.array(rows), np.array(lens, np.uint16), np.array(ifi, np.uint32))
        for a in out:
            a.setflags(write=False)
        _CACHE[("sweep", v6)] = out
    return _CACHE[("sweep", v6)]


def sha256(*arrays) -> bytes:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.digest()


def fixture_legs():
    """[(name, br, v6, frames, lens, ifindex)]: what tests/golden/br_shift.npz records, in order:
    the corpus per (family, BR), then the sweep per family (br1)."""
    legs = []
    for v6 in (False, True):
        for br in BRS:
            fr, ln, ifi, _, _ = shift_corpus(v6)[br]
            legs.append((corpus_name(br, v6), br, v6, fr, ln, ifi))
    for v6 in (False, True):
        fr, ln, ifi = truncation_sweep(v6)
        legs.append((sweep_name(v6), "br1", v6, fr, ln, ifi))
    return legs


def oracle(name):
    """((action, verdict, egress, stats), frames out) of the oracle router on the fixture leg
    `name` ("corpus_<v6>_<br>", "sweep_<v6>"), computed once and left unchanged."""
    if ("oracle", name) not in _CACHE:
        _, br, v6, frames, lens, ifidx = next(leg for leg in fixture_legs() if leg[0] == name)
        out = frames.copy()
        res = orc.br_process(out, lens, ifidx, T.br_config(br, v6), orc.hop_key(T.KEYS[1]))
        for a in res + (out,):
            a.setflags(write=False)
        _CACHE[("oracle", name)] = (res, out)
    return _CACHE[("oracle", name)]


def corpus_name(br, v6):
    return "corpus_%d_%s" % (v6, br)


def sweep_name(v6):
    return "sweep_%d" % v6
