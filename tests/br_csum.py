"""Forwardable frames aimed at every carry and sign edge of the router's incremental checksums.

rewrite() in hfv_br_kernel.hip (and the oracle's) must give, bit for bit, what the reference's
rewrite.h gives for the IPv4 header checksum and the UDP checksum over IPv4 and IPv6:

    csum = ~check + residual + 1;   FOLD_CHECKSUM(csum);   check = csum;

  * the residual is a u64 sum mod 2^64 of little-endian loads, new fields minus old ones;
  * `check` is a u16, promoted to int before `~`, so `~check` is a negative int that converts to
    u64 by sign extension: 2^64 - 1 - check (the complement is NOT taken at 16 bits);
  * FOLD_CHECKSUM folds twice, which does not reduce a 64-bit value, and its `if (csum == 0)
    csum = 0xffff` looks at all 64 bits after `~`: dead, so 0x0000 is a possible result.

With R the true signed sum "new minus old", C the incoming check field (both as the little-endian
loads the code makes) and D = R - C, the stored field is a function of D alone:
cs = D mod 2^64, f1 = (cs & 0xffff) + (cs >> 16), f2 = (f1 & 0xffff) + (f1 >> 16), result =
~f2 & 0xffff.  An ordinary one's-complement update gives full(D) = 0xffff - (D mod 65535) (in
1..0xffff); the rule differs from it only for D > 0 with D = 0 (mod 65535) (0x0000, not 0xffff),
for D >= 2^32 whose f2 keeps bit 16 (one off), and for some D <= -2^32 (one off; for -2^32 < D < 0
the two always agree: with m = -D = 65536 q + r, 1 <= r <= 65536, both give q + r or q + r - 65535).

This module is a plain-integer model of that rule (Python ints, no C, no HIP), the classes of D
it distinguishes, five wrong rules a port could have instead (VARIANTS), and a corpus of frames
whose D is solved for with the model: every frame is a PTF hop input of br1 (`direct`: next hop a
link, `sibling`: a sibling BR, `ipfwd`: an IP forward; all four path kinds) with the fields the
router reads but never checks set so that D lands on a target: the incoming check field, the UDP
source port, the source address, TTL / hop limit.  |R| beyond what the topology's addresses give
needs other link addresses, so some frames run under copies of br1's tables with the link,
sibling, internal and ingress addresses replaced (csum_config: "mid", "hi", "lo").

The model only classifies and aims; the judges are the reference program and the oracle
(tests/test_br_csum.py, tests/test_gpu_br_csum.py).  Test infrastructure only.
"""
import struct

import numpy as np

import br_fuzz as F
import br_shift as S
import br_topo as T
import orc
import scion_hfv as hfv

MAC = S.MAC
SLOT = 256
M64 = (1 << 64) - 1
KINDS = ("ip4", "udp4", "udp6")                  # checksum kinds
NEXT_HOPS = ("link", "sibling", "ipfwd")
VARIANTS = (1, 2, 3, 4, 5)
VARIANT_NAMES = {1: "a third fold", 2: "zero test on the low 16 bits", 3: "~C taken at 16 bits, zero-extended",
                 4: "cs truncated to 32 bits", 5: "RFC 1624 16-bit update"}
FORWARD = hfv.VERDICT["SCION_FORWARD"]


# ---- the model ----------------------------------------------------------------------------------

def le(b, off, size):
    return int.from_bytes(bytes(b[off:off + size]), "little")


def layout(frame):
    """(v6, check offsets {kind: off}, fields {kind: [(off, size)]}) of a frame by the parser's rule
    (br_shift.field_offsets): what each checksum's residual covers."""
    proto = struct.unpack_from(">H", frame, 12)[0]
    v6 = proto == 0x86DD
    assert v6 or proto == 0x0800
    ip = 14
    udp = ip + (40 if v6 else 4 * (frame[14] & 15))
    o = S.field_offsets(frame)
    addrs = [(ip + 8 + 4 * i, 4) for i in range(8)] if v6 else [(ip + 12, 4), (ip + 16, 4)]
    path = [(udp, 2), (udp + 2, 2), o["meta"], o["seg0"]] + ([o["seg1"]] if o["seg1"] else [])
    if v6:
        return True, {"udp6": udp + 6}, {"udp6": addrs + path}
    return False, {"ip4": ip + 10, "udp4": udp + 6}, {"ip4": addrs + [(ip + 8, 1)], "udp4": addrs + path}


def residuals(fin, fout):
    """{kind: (R, C)} of one forwarded frame: R = sum over the checksum's fields of (little-endian
    load from the output - load from the input), C = the input's check field."""
    _, checks, fields = layout(fin)
    return {k: (sum(le(fout, o, s) - le(fin, o, s) for o, s in fields[k]), le(fin, checks[k], 2)) for k in checks}


def fold(c):
    return (c & 0xFFFF) + (c >> 16)


def full(D):
    """An ordinary one's-complement update: 0xffff - (D mod 65535), in 1..0xffff."""
    return 0xFFFF - D % 65535


def rule(R, C, variant=0):
    """(cs, f1, f2, stored check field) by the reference's rule, or by wrong rule `variant`."""
    D = R - C
    cs = D & M64                                  # ~C + R + 1 with ~C = 2^64 - 1 - C
    if variant == 3:
        cs = ((~C & 0xFFFF) + R + 1) & M64
    if variant == 4:
        cs &= 0xFFFFFFFF
    if variant == 5:                              # HC' = ~(~HC + ~m + m') in 16-bit one's complement
        s = (D - 1) % 65535 + 1                   # the folded sum: never 0, the ~m terms are not
        return cs, s, s, 0xFFFF - s
    f1 = fold(cs)
    f2 = fold(f1)
    f = fold(f2) if variant == 1 else f2
    c = ~f & M64
    if (c & 0xFFFF if variant == 2 else c) == 0:
        c = 0xFFFF
    return cs, f1, f2, c & 0xFFFF


def classify(R, C):
    """The classes of D = R - C the rule distinguishes."""
    D = R - C
    _, f1, f2, res = rule(R, C)
    return {"D": D, "sign": (D > 0) - (D < 0), "band": 0 if abs(D) < 1 << 16 else 1 if abs(D) < 1 << 32 else 2,
            "full": res == full(D), "bit16": D > 0 and bool(f2 & 0x10000), "f1hi": f1 >> 16 if D > 0 else None,
            "result": res, "C": C}


BANDS = ("< 2^16", "< 2^32", ">= 2^32")
CLASSES = (("D = 0", lambda c: c["sign"] == 0),) + tuple(
    ("D %s 0, |D| %s" % ("<>"[s > 0], BANDS[b]), lambda c, s=s, b=b: c["sign"] == s and c["band"] == b)
    for s in (-1, 1) for b in range(3)) + (
    ("D > 0, D = 0 mod 65535", lambda c: c["sign"] > 0 and c["D"] % 65535 == 0),
    ("D > 0, bit 16 after fold 2", lambda c: c["bit16"]),
    ("D < 0, result 0x0000", lambda c: c["sign"] < 0 and c["result"] == 0),
    ("two folds != full fold", lambda c: not c["full"]),
    ("result 0x0000", lambda c: c["result"] == 0x0000), ("result 0xffff", lambda c: c["result"] == 0xFFFF),
    ("result 0x0001", lambda c: c["result"] == 0x0001), ("result 0xfffe", lambda c: c["result"] == 0xFFFE),
    ("C 0x0000", lambda c: c["C"] == 0x0000), ("C 0xffff", lambda c: c["C"] == 0xFFFF))
CLASS_NAMES = tuple(n for n, _ in CLASSES)


def classes_of(R, C):
    c = classify(R, C)
    return [n for n, p in CLASSES if p(c)]


def next_hop_kind(cfg, fin, fout):
    """link / sibling / ipfwd from the tables in plain Python: an IP forward keeps both addresses;
    otherwise the new destination is an egress entry's remote address."""
    v6 = layout(fin)[0]
    w, src, dst = (16, 22, 38) if v6 else (4, 26, 30)
    if fin[src:src + w] == fout[src:src + w] and fin[dst:dst + w] == fout[dst:dst + w]:
        return "ipfwd"
    ext = {bytes(cfg.egress[i].remote)[:w]: bool(cfg.egress[i].fwd_external) for i in range(cfg.n_egress)}
    return "link" if ext[bytes(fout[dst:dst + w])] else "sibling"


# ---- tables -------------------------------------------------------------------------------------

TABLES = ("base", "mid", "hi", "lo")
# address bytes after the first (a tag that keeps the entries apart): new destination, new source,
# the ingress address (the frame's old destination).  Little-endian loads: the last byte of a word
# is its top byte.
_FILL = {
    False: {"mid": ([0xFF, 0xFF, 0x7F], [0xFF, 0xFF, 0x7F], [0] * 3),         # new - old about 2^32
            "hi": ([0xFF] * 3, [0xFF] * 3, [0] * 3),                          # about 2^33
            "lo": ([0] * 3, [0] * 3, [0xFF] * 3)},                            # about -2^32
    True: {"hi": ([0xFF] * 7 + [0] * 8, [0xFF] * 3 + [0] * 12, [0] * 15),    # about 3 * 2^32
           "lo": ([0] * 15, [0] * 15, [0xFF] * 15)},                          # about -4 * 2^32
}


def tables(v6):
    return ("base",) + tuple(t for t in TABLES if t in _FILL[v6])


def csum_config(v6, table):
    """br1's tables (topology.br_config), for "mid", "hi" and "lo" with every link, sibling, internal
    and ingress address replaced: same interfaces, routes and ports, other address bytes."""
    if table == "base":
        return T.br_config("br1", v6)
    nd, ns, ing = _FILL[v6][table]
    c = hfv.BrConfig()
    plen = 128 if v6 else 32
    internal = {5: bytes([0x45] + ns), 7: bytes([0x47] + ns)}                  # br1's veth5, veth7
    sibling = {"br2": (bytes([0x32] + nd), 5, 4), "br3": (bytes([0x33] + nd), 7, 6)}
    for veth, addr in internal.items():
        c.add_int_iface(veth, addr, 31002)
        c.add_tx_port(veth)
    ext = ((1, 1, 0), (2, 3, 2))                                              # ifid, veth, remote veth
    for ifid, veth, _ in ext:
        c.add_ingress(veth, bytes([0x50 + ifid] + ing), 50000, ifid)
        c.add_tx_port(veth)
    for ifid in range(1, 7):
        if ifid <= 2:
            c.add_egress_link(ifid, bytes([0x20 + ifid] + ns), 50000, bytes([0x10 + ifid] + nd), 50000)
        else:
            c.add_egress_sibling(ifid, sibling["br2" if ifid <= 4 else "br3"][0], 31002)
    for ifid, veth, rveth in ext:
        c.add_route(bytes([0x10 + ifid] + nd), plen, veth, T.MAC[veth], T.MAC[rveth])
    for addr, veth, peer in sibling.values():
        c.add_route(addr, plen, veth, T.MAC[veth], T.MAC[peer])
    return c


def ingress_addr(v6, table, ifid=1):
    return bytes([0x50 + ifid] + _FILL[v6][table][2])


# ---- targets ------------------------------------------------------------------------------------

def _find_negative(pred):
    """The first D = -(2^32 q1 + 65536 q0 + r) just below -2^32 q1 that satisfies pred, by the model.
    With lo = -r mod 2^16 the low half of f1 is L = lo - q0 - 1 and that of f2 is L - 1 - q1 + carry,
    each mod 2^16: for lo just above q0 the second goes below zero and the one's-complement borrow
    is lost, so the result is one below full(D): 0 for q1 = 1, 1 for q1 = 2, ..."""
    for q1 in (1, 2, 3):
        for q0 in range(32):
            for lo in range(1, 40):
                D = -((q1 << 32) + 65536 * q0 + (65536 - lo))
                if pred(D, rule(D, 0)[3]):
                    return D
    raise AssertionError("no such D")


NEG_ZERO = _find_negative(lambda D, r: r == 0)
NEG_ONE_OFF = -(1 << 33)           # q1 = 1, q0 = 0xffff, lo = 0: no carry, L = 0, result 0x0001 where full(D) is 0x0002
# (name, D or None for "whatever R - C gives", forced C or None)
TARGETS = (
    ("zero", 0, None), ("+1", 1, None), ("-1", -1, None), ("+65535", 65535, None), ("-65535", -65535, None),
    ("+65536", 65536, None), ("-65536", -65536, None), ("+65534", 65534, None), ("-65534", -65534, None),
    ("mod 65535, >= 2^32", 65535 * 65538, None),
    ("bit 16, f1 >> 16 = 1", 0x1FFFE0001, None), ("bit 16, f1 >> 16 = 2, below 2^33", 0x1FFFFFFFF, None),
    ("bit 16, f1 >> 16 = 2, above 2^33", 0x20000FFFF, None),
    ("negative, result 0", NEG_ZERO, None), ("negative, one off", NEG_ONE_OFF, None),
    ("negative, result 0, second", -8014733896, None), ("negative, one off, second", -28182868007, None),
    ("+small", 0x1234, None), ("-small", -0x1234, None), ("+mid", 0x00A34567, None), ("-mid", -0x12345678, None),
    ("+big", 0x123456789, None), ("-big", -0x123456789, None),
    ("C 0, +", 0x2345, 0x0000), ("C 0, -", -0x0B00000, 0x0000), ("C ffff, +", 0x00B00000, 0xFFFF),
    ("C ffff, -", -0x2345, 0xFFFF), ("C 0, D 0", 0, 0x0000), ("C 0, as it comes", None, 0x0000),
    ("C ffff, as it comes", None, 0xFFFF), ("C ffff, -65536", -65536, 0xFFFF),
)
EDGE_TARGETS = tuple(n for n, _, _ in TARGETS[:17])
TTLS = (0, 1, 2, 64, 255)
SCENARIO = {"link": "direct", "sibling": "sibling", "ipfwd": "ipfwd"}

_CACHE = {}


def bases(v6):
    """{(scenario, path kind): (frame, ingress ifindex)}: the PTF inputs as br1 sees them."""
    if ("bases", v6) not in _CACHE:
        seen, out = iter(F.ptf_cases(v6, MAC)), {}
        mine = [(i, f) for b, i, f in F.hop_inputs({b: T.OracleBR(T.br_config(b, v6)) for b in S.BRS}, v6, MAC,
                                                   seeds=(0x1234,)) if b == "br1"]
        assert len(mine) == 12
        for (name, kind, _, _, _, _, _), (ifi, f) in zip(seen, mine):   # br1 sees each case exactly once
            out[(name, kind)] = (f, ifi)
        assert sorted({n for n, _ in out}) == ["direct", "ipfwd", "sibling"]
        _CACHE[("bases", v6)] = out
    return _CACHE[("bases", v6)]


def _oracle_one(frame, ifi, cfg):
    buf, lens = T.to_slots([frame], slot=SLOT)
    a, v, e, _ = orc.br_process(buf, lens, np.array([ifi], np.uint32), cfg, orc.hop_key(T.KEYS[1]))
    return int(v[0]), buf[0, :len(frame)].tobytes()


def _set(frame, off, value: bytes):
    return frame[:off] + value + frame[off + len(value):]


def _probe(v6, scenario, pkind, table, ttl):
    """The base frame made forwardable under `table` (its destination the table's ingress address)
    with TTL / hop limit `ttl`, and the oracle's output for it: the new field values, which do not
    depend on the fields the solver sets (link, sibling) or follow them (IP forward)."""
    key = ("probe", v6, scenario, pkind, table, ttl)
    if key not in _CACHE:
        frame, ifi = bases(v6)[(scenario, pkind)]
        if table != "base":
            frame = _set(frame, 38 if v6 else 30, ingress_addr(v6, table))
        if ttl is not None:
            frame = _set(frame, 21 if v6 else 22, bytes([ttl]))
        verdict, out = _oracle_one(frame, ifi, csum_config(v6, table))
        _CACHE[key] = (frame, ifi, out) if verdict == FORWARD else None
    return _CACHE[key]


def solve(v6, nh, pkind, kind, D, C, ttl=None, salt=0):
    """(table, frame, ifindex) whose checksum `kind` has R - C = D (D None: C forced, D as it comes)
    under the first table that can reach it, or None.  Linear in the free fields: for a link or a
    sibling the new addresses, ports and TTL come from the tables, so R = Rz - (source address
    words + source port [udp]) with Rz the residual at zeroed free fields; an IP forward keeps them,
    so only C is free."""
    for table in tables(v6) if nh != "ipfwd" else ("base",):
        p = _probe(v6, SCENARIO[nh], pkind, table, ttl)
        if p is None:
            continue
        frame, ifi, out = p
        R = residuals(frame, out)[kind][0]
        _, checks, _ = layout(frame)
        src, nw = (22, 4) if v6 else (26, 1)
        udp = 54 if v6 else 34
        if nh == "ipfwd":
            c = C if D is None else R - D
            if not 0 <= c <= 0xFFFF or (C is not None and c != C):
                continue
            return table, _set(frame, checks[kind], struct.pack("<H", c)), ifi
        free = [("w%d" % i, 0xFFFFFFFF, 0) for i in range(nw)]
        Rz = R + sum(le(frame, src + 4 * i, 4) for i in range(nw))
        if kind != "ip4":
            Rz += le(frame, udp, 2)
            free.append(("sport", 0xFFFF, 1 + (0x51ED * (salt + 3)) % 0xFFFD))
        if D is None:
            D = Rz - C - 0x01020304 - 0x4321                       # an ordinary source address and port
        if C is None:
            free.append(("C", 0xFFFF, 1 + (0x9E37 * (salt + 1)) % 0xFFFD))
        X = Rz - D - (C or 0)
        if not 0 <= X <= sum(cap for _, cap, _ in free):
            continue
        val = {}
        for name, cap, pref in reversed(free):                     # the 16-bit fields take their ordinary value,
            val[name] = min(X, pref)                               # the address words the bulk,
            X -= val[name]
        for name, cap, _ in free:                                  # and whatever is left tops the fields up
            add = min(X, cap - val[name])
            val[name] += add
            X -= add
        assert X == 0
        for i in range(nw):
            frame = _set(frame, src + 4 * i, struct.pack("<I", val["w%d" % i]))
        if "sport" in val:
            frame = _set(frame, udp, struct.pack("<H", val["sport"]))
        frame = _set(frame, checks[kind], struct.pack("<H", val.get("C", C)))
        return table, frame, ifi
    return None


def plan(v6):
    """[(target name, next hop, path kind, checksum kind, D, C, ttl)]: every target for every next-hop
    kind and checksum kind, the path kind rotating; for the IP forward each TTL / hop limit."""
    out = []
    kinds = ("udp6",) if v6 else ("ip4", "udp4")
    for t, (name, D, C) in enumerate(TARGETS):
        for h, nh in enumerate(NEXT_HOPS):
            for k, kind in enumerate(kinds):
                out.append((name, nh, F.KINDS[(t + h + k) % 4], kind, D, C, None))
    for t, ttl in enumerate(TTLS):
        for k, kind in enumerate(kinds):
            out.append(("ttl %d" % ttl, "ipfwd", F.KINDS[(t + k) % 4], kind, -0x1234 - t, None, ttl))
            out.append(("ttl %d, C 0" % ttl, "ipfwd", F.KINDS[(t + k + 1) % 4], kind, None, 0, ttl))
    if not v6:          # TTL 0 becomes 255: the one IP forward whose header residual is positive
        for t, D in enumerate((0, 1, 255, -65280)):
            out.append(("ttl 0, D %d" % D, "ipfwd", F.KINDS[t], "ip4", D, None, 0))
    return out


def corpus(v6):
    """{table: (frames u8[n, 256], lens u16[n], ifindex u32[n], [(target, next hop, path kind, checksum
    kind aimed at, D aimed at)])}, built once and left unchanged.  A target no table reaches for a
    next-hop kind gives no frame; PLACEMENT in tests/test_br_csum.py is what holds the coverage."""
    if ("corpus", v6) not in _CACHE:
        per = {t: ([], [], []) for t in tables(v6)}
        for salt, (name, nh, pkind, kind, D, C, ttl) in enumerate(plan(v6)):
            got = solve(v6, nh, pkind, kind, D, C, ttl, salt)
            if got is None:
                continue
            table, frame, ifi = got
            per[table][0].append(frame), per[table][1].append(ifi), per[table][2].append((name, nh, pkind, kind, D))
        out = {}
        for table, (fl, ifi, meta) in per.items():
            frames, lens = T.to_slots(fl, slot=SLOT)
            out[table] = (frames, lens, np.array(ifi, np.uint32), tuple(meta))
            for a in out[table][:3]:
                a.setflags(write=False)
        _CACHE[("corpus", v6)] = out
    return _CACHE[("corpus", v6)]


def legs():
    """[(name, v6, table, cfg, frames, lens, ifindex, meta)] in the fixture's order."""
    return [("%s_%s" % ("v6" if v6 else "v4", t), v6, t, csum_config(v6, t)) + corpus(v6)[t]
            for v6 in (False, True) for t in tables(v6)]


def oracle(name):
    """((action, verdict, egress, stats), frames out) of the oracle router on leg `name`, once."""
    if ("oracle", name) not in _CACHE:
        _, _, _, cfg, frames, lens, ifidx, _ = next(leg for leg in legs() if leg[0] == name)
        out = frames.copy()
        res = orc.br_process(out, lens, ifidx, cfg, orc.hop_key(T.KEYS[1]))
        for a in res + (out,):
            a.setflags(write=False)
        _CACHE[("oracle", name)] = (res, out)
    return _CACHE[("oracle", name)]


def fixture_legs(g):
    """[(name, cfg, frames, lens, ifindex, (action, verdict, egress, stats), frames out)] as
    tests/golden/br_csum.npz holds them: inputs, tables and results, nothing regenerated."""
    names = [str(n) for n in g["names"]]
    out = []
    for t, name in enumerate(names):
        sel = g["table"] == t
        cfg = hfv.BrConfig.from_buffer_copy(g["cfgs"][t].tobytes())
        frames = np.ascontiguousarray(g["frames"][sel])
        want = (g["action"][sel], g["verdict"][sel], g["egress"][sel], g["stats"][t])
        out.append((name, cfg, frames, g["lens"][sel], g["ifidx"][sel], want, frames ^ g["xor"][sel]))
    return out


def placement():
    """{(checksum kind, next-hop kind, class): frames of the corpus that land there}, by the model on
    the oracle's outputs; both checksums of an IPv4 frame count, whichever one it was aimed at."""
    table = {(k, h, c): 0 for k in KINDS for h in NEXT_HOPS for c in CLASS_NAMES}
    for name, _, _, cfg, frames, lens, _, _ in legs():
        out = oracle(name)[1]
        for i in range(len(frames)):
            fin, fout = bytes(frames[i, :lens[i]]), bytes(out[i, :lens[i]])
            nh = next_hop_kind(cfg, fin, fout)
            for kind, (R, C) in residuals(fin, fout).items():
                for c in classes_of(R, C):
                    table[(kind, nh, c)] += 1
    return table


def count_classes(frames, lens, out, forwarded):
    """(frames per class name, frames the model gets wrong, {variant: frames it changes}) over the
    forwarded frames of a batch: both check fields of every frame by the model against `out`."""
    counts, wrong, variants, n = {c: 0 for c in CLASS_NAMES}, 0, {v: 0 for v in VARIANTS}, 0
    for i in np.nonzero(forwarded)[0]:
        fin, fout = bytes(frames[i, :lens[i]]), bytes(out[i, :lens[i]])
        _, checks, _ = layout(fin)
        hit, bad, var = set(), False, set()
        for kind, (R, C) in residuals(fin, fout).items():
            want = rule(R, C)[3]
            bad |= le(fout, checks[kind], 2) != want
            hit |= set(classes_of(R, C))
            var |= {v for v in VARIANTS if rule(R, C, v)[3] != want}
        n += 1
        wrong += bad
        for c in hit:
            counts[c] += 1
        for v in var:
            variants[v] += 1
    return n, counts, wrong, variants


FUZZ_BATCHES = tuple((br, v6) for v6 in (False, True) for br in S.BRS)   # test_gpu_br.test_fuzz_parity


def fuzz_recount(br, v6):
    """count_classes over one 20000-frame batch of test_gpu_br.test_fuzz_parity, by the oracle."""
    frames, lens, ifidx = F.fuzz_batch(S.hop_inputs(v6), br, v6, 20000, seed=100 + v6, payload_max=1500)
    out = frames.copy()
    _, v, _, _ = orc.br_process(out, lens, ifidx, T.br_config(br, v6), orc.hop_key(T.KEYS[1]))
    return count_classes(frames, lens, out, v == FORWARD)
