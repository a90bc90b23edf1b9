"""Shared by test_frames_hostmem.py and test_gpu_frames_hostmem.py: the run-again rule of
hfv_verify_frames_host restated in plain Python, and the corpus both modules run.

The rule.  The pageable path copies the first `window` bytes of each slot to the device and parses
min(len, slot, window) bytes of the frame.  The parser (br/src/bpf/parser.h:45-204, restated in
parse() below from test_frames_host.ref_parse, with the compare that stopped it reported) stops in
one of three ways:
  ("ok",)          every header was found;
  ("value", what)  a field's value ends the parse (EtherType, IHL, IP protocol, SCION version, path
                   type): no further byte changes that;
  ("bound", x)     the next header would end at x, past the bytes present.
A frame whose clamped parse stops at a bound while more of the frame lies past the window
(min(len, slot) > window) is undecided and is run again with its whole slot; every other frame's
clamped result is final.  Test infrastructure only; independent of the C and HIP code."""
import functools
import struct

import numpy as np

import br_fuzz as F
import br_shift as S
import br_topo as T
import frames_rx_ref as R
from scion_hfv import packets as P

OK, PARSE_ERROR, NOT_SCION, NOT_IMPLEMENTED = 0, 17, 26, 34
WINDOWS = (64, 120, 128, 136, 256)
SLOT = 1024                      # the corpus' slot: the long-path frames are ~700 bytes
# The shortest parse that succeeds ends at byte 94: Ethernet 14 + IPv4 20 + UDP 8 + SCION 28 + host
# addresses 8 + PathMeta 4 + a hop field 12 (no info field) -- no frame is OK inside 64 bytes.
MIN_OK_END = 14 + 20 + 8 + 28 + 8 + 4 + 12


def parse(f: bytes, end: int):
    """(status, inf_off, hf_off, stop) of the parser over f[:end]."""
    def out(status, stop, inf=0, hf=0):
        return status, inf, hf, stop

    data = 14
    if data > end:
        return out(NOT_SCION, ("bound", data))
    proto = struct.unpack_from(">H", f, 12)[0]
    if proto == 0x0800:
        ip = data
        data += 20
        if data > end:
            return out(NOT_SCION, ("bound", data))
        skip = 4 * (f[ip] & 0x0F) - 20
        if skip < 0 or skip > 40:
            return out(NOT_SCION, ("value", "ihl"))
        data += skip
        if f[ip + 9] != 17:
            return out(NOT_SCION, ("value", "protocol"))
    elif proto == 0x86DD:
        ip = data
        data += 40
        if data > end:
            return out(NOT_SCION, ("bound", data))
        if f[ip + 6] != 17:
            return out(NOT_SCION, ("value", "nexthdr"))
    else:
        return out(NOT_SCION, ("value", "ethertype"))
    data += 8
    if data > end:
        return out(NOT_SCION, ("bound", data))
    sc = data
    data += 28
    if data > end:
        return out(PARSE_ERROR, ("bound", data))
    if f[sc] >> 4 != 0:
        return out(NOT_IMPLEMENTED, ("value", "version"))
    data += P.ref_host_addr_len(f[sc + 9])
    if data > end:
        return out(PARSE_ERROR, ("bound", data))
    if f[sc + 8] != 1:
        return out(NOT_IMPLEMENTED, ("value", "path type"))
    meta = data
    data += 4
    if data > end:
        return out(PARSE_ERROR, ("bound", data))
    h = struct.unpack_from(">I", f, meta)[0]
    num_inf = sum(1 for sh in (12, 6, 0) if (h >> sh) & 0x3F)
    curr_inf, curr_hf = h >> 30, (h >> 24) & 0x3F
    inf = data + 8 * curr_inf
    hf = data + 8 * num_inf + 12 * curr_hf
    if inf + 8 > end:
        return out(PARSE_ERROR, ("bound", inf + 8), inf)
    if curr_inf + 1 < num_inf and inf + 16 > end:
        return out(PARSE_ERROR, ("bound", inf + 16), inf)
    if hf + 12 > end:
        return out(PARSE_ERROR, ("bound", hf + 12), inf, hf)
    return out(OK, ("ok",), inf, hf)


def classify(row: bytes, ln: int, slot: int, window: int):
    """("final" | "again", the clamped parse, the whole-frame parse) of one frame in its slot."""
    end = min(ln, slot)
    clamped = parse(row, min(end, window))
    again = clamped[3][0] == "bound" and end > window
    return ("again" if again else "final"), clamped, parse(row, end)


def retried(frames, lens, window):
    """bool[n]: the frames the pageable path runs again at this window."""
    slot = frames.shape[1]
    return np.array([classify(bytes(frames[i]), int(lens[i]), slot, window)[0] == "again" for i in range(len(frames))])


CLASSES = ("final ok", "final value, bytes past the window", "again then ok", "again then error")


def placement(frames, lens, window):
    """{class: count} over the frames (frames of no class -- short ones, final bound stops -- are
    not counted)."""
    slot = frames.shape[1]
    t = dict.fromkeys(CLASSES, 0)
    for i in range(len(frames)):
        kind, clamped, whole = classify(bytes(frames[i]), int(lens[i]), slot, window)
        if kind == "again":
            t[CLASSES[2] if whole[0] == OK else CLASSES[3]] += 1
        elif clamped[3][0] == "ok":
            t[CLASSES[0]] += 1
        elif clamped[3][0] == "value" and min(int(lens[i]), slot) > window:
            t[CLASSES[1]] += 1
    return t


def _non_scion(v4_frame: bytes, v6_frame: bytes):
    """Frames a value check ends, padded past every window: [(name, frame)]."""
    pad = bytes(range(256)) * 2
    out = []

    def add(name, base, at, value):
        g = bytearray(base + pad)
        g[at] = value
        out.append((name, bytes(g)))

    add("ethertype arp", v4_frame, 13, 0x06)
    add("ipv4 tcp", v4_frame, 14 + 9, 6)
    add("ipv4 ihl 4", v4_frame, 14, 0x44)
    add("ipv6 icmp", v6_frame, 14 + 6, 58)
    add("version 1 v4", v4_frame, S.scion_offset(v4_frame, False), 0x10)
    add("version 1 v6", v6_frame, S.scion_offset(v6_frame, True), 0x10)
    add("path type 2 v4", v4_frame, S.scion_offset(v4_frame, False) + 8, 2)
    add("path type 2 v6", v6_frame, S.scion_offset(v6_frame, True) + 8, 2)   # byte 70: past a 64-byte window
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """(frames u8[n, SLOT], lens u16[n], ifindex u32[n], names): br1's window-edge frames of
    br_shift (every third IPv4 one, every IPv6 one), the long-path frames of both families whole,
    with one MAC bit flipped and cut one byte short of the hop field's end, every third IPv4-options
    frame, the non-SCION frames above, and every truncation of one valid frame.  Read-only, a few
    hundred frames; the last frame is a long-path one (undecided at every window below its hop
    field)."""
    rows, ifi, names = [], [], []

    def add(name, frame, ifindex, ln=None):
        rows.append((frame, len(frame) if ln is None else ln))
        ifi.append(ifindex)
        names.append(name)

    for v6 in (False, True):
        fr, ln, ix, _, _ = S.shift_corpus(v6)["br1"]
        for i in range(0, len(fr), 1 if v6 else 3):
            add("shift", bytes(fr[i, :ln[i]]), int(ix[i]))
    fr, ln, ix, _ = F.options_shift_batch(R.hop_inputs(False))
    for i in range(1, len(fr), 3):
        add("options", bytes(fr[i, :ln[i]]), int(ix[i]))
    base = {v6: next(f for b, _, f in R.hop_inputs(v6) if b == "br1") for v6 in (False, True)}
    ifi1 = next(i for b, i, _ in R.hop_inputs(False) if b == "br1")
    for name, f in _non_scion(base[False], base[True]):
        add(name, f, ifi1)
    for ln in range(len(base[False]) + 1):
        add("truncated", base[False], ifi1, ln)
    longs = [(f, i) for v6 in (False, True) for f, i in F.long_path_frames(v6, R.MAC)]
    for f, i in longs:
        g = bytearray(f)
        g[parse(f, len(f))[2] + 6 + len(rows) % 6] ^= 1 << len(rows) % 8   # one MAC bit
        add("long bad mac", bytes(g), i)
    for f, i in longs:
        add("long cut", f, i, parse(f, len(f))[2] + 11)
    for f, i in longs:
        add("long", f, i)
    frames = np.zeros((len(rows), SLOT), np.uint8)
    lens = np.zeros(len(rows), np.uint16)
    for k, (f, ln) in enumerate(rows):
        frames[k, :len(f)] = np.frombuffer(f, np.uint8)
        lens[k] = ln
    ifidx = np.array(ifi, np.uint32)
    for a in (frames, lens, ifidx):
        a.setflags(write=False)
    return frames, lens, ifidx, tuple(names)


def oracle(frames, lens, n, internal, hop_keys, valid, keysel):
    """(bitmap words, status) by hfv_frame_extract per frame and the record checker: the judge of
    test_gpu_frames_fused.py."""
    internal = np.asarray(internal, dtype=bool)
    internal = internal[:n] if internal.ndim else np.broadcast_to(internal, (n,))
    st, inf, hf = R.frame_extract(np.ascontiguousarray(frames[:n]), lens[:n], internal)
    return R.oracle_bits(st, inf, hf, hop_keys, valid, keysel), st
