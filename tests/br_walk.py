"""The SCION path walk of the router (parse_scion_path, scion_as_ingress, scion_as_egress, the info
field step after a segment switch, the PathMeta and SegID stores of rewrite_scion_path and the order
"read the MAC input, then rewrite") restated in plain integers, and a designed corpus that puts a
frame on every CurrINF, CurrHF and SegLen edge of it.

TEST INFRASTRUCTURE ONLY.

The model.  walk(path, plen, ...) follows the reference text (br/src/bpf/parser.h:153-204,
path_processing.h:39-152, rewrite.h:123-146, xdp.c:129-245) over the bytes from the PathMeta word on,
with BR 1's tables of the test topology reduced to what the walk needs of them: which AS interface a
frame came in on, and what the egress map says about an interface ID.  It depends neither on the CPU
checker nor on the HIP code.  Offsets are relative to the PathMeta word.  It gives num_inf, num_hf, the
info and hop field offsets, whether ingress switched, the PathMeta word and the SegIDs stored and
where, the (INF, HF) pair of the deferred MAC check with its beta, d = INF - HF of that pair, the
verdict, the egress ifindex and every byte of the path after the rewrite.  geometry() is the same
arithmetic on (seg0, num_inf, CurrINF, CurrHF) alone, for enumerating the whole space.

What the enumeration shows (tests/test_br_walk.py asserts it):
  * of the rewrite's two SegID stores only the one at INF+2 can land in the hop field under check, at
    d in {0, 4, 8}; the store at INF+10 needs a switch, a switch needs CurrHF + 1 = seg0 * k with
    k = min(CurrINF, 2) + 1, and then INF+10 is never inside HF..HF+11 on a frame that gets past the
    NOT_IMPLEMENTED test;
  * the bare `return 0` of process_packet and of scion_as_egress (INF+16 past the end after a switch)
    cannot be reached: after a switch the switched hop field ends behind INF+16, so the frame is a
    PARSE_ERROR first.
(The reference adds seg0 once for CurrINF >= 1 and once more for >= 2, so k is 3 for CurrINF 3 too.)

The wrong rules.  walk(rule=N) and mac_ok(rule=N) restate the wrong steps of -DHFV_MUT_PATHWALK=N
(csrc/hfv_br_kernel.hip, `make pathwalk`); locate(rule=9) the one of frame_locate.

The corpus.  corpus(v6) is built once per family for BR 1, 1024-byte slots:
  base      LAYOUTS x CurrINF 0..3 x the edge CurrHF values x every Cons combination of the info fields
            present x DIRECTIONS.  The hop field(s) the router reads carry the interface IDs that pass
            the interface checks for the Cons bits that govern them (bits of hop field bytes where
            CurrINF points past the info fields).  Where the model says the frame is rewritten with a
            MAC check whose SegID and timestamp lie outside the checked hop field ("case A"), the MAC
            is made valid by the reference's rule;
  flip      two one-bit-flipped twins of every case-A frame, the flipped field rotating over SegID,
            timestamp, ExpTime, ConsIngress, ConsEgress and the six MAC bytes (an interface ID is
            flipped only where the walk still reaches the MAC check);
  dontcare  one twin that differs in hop field byte 0 bits 2..7 or info field byte 1 only;
  alert     a twin of every case-A frame with router alert flags on the hop field scion_as_ingress
            reads, or (a switched frame) on the one scion_as_egress reads;
  short     the frames whose CurrHF + 1 is both num_hf and seg_end, once more without payload;
  overlap   the MAC input / SegID store overlaps (OVERLAP below), searched constants;
  trunc     one forwarding frame per switch kind and per overlap kind cut at every length from the
            PathMeta word to HF + 24.
Every expectation of the tests comes from the CPU checker pinned to the reference program, from the
fixture tests/golden/br_walk.npz or from this model, never from the library."""
import collections
import functools
import struct

import numpy as np

import orc
import scion_hfv as hfv
from scion_hfv import packets as P
from scion_hfv import topology as TP

V = hfv.VERDICT
SLOT = 1024
KEY = TP.KEYS[1]
HK = orc.hop_key(KEY)
LAYOUTS = ((3, 0, 0), (2, 3, 0), (2, 2, 2), (0, 3, 0), (3, 0, 2), (1, 1, 1), (1, 3, 0), (4, 4, 0), (16, 16, 16),
           (21, 1, 1), (63, 2, 0), (1, 63, 0), (0, 0, 0))
FILLER_HOPS = 3                   # hop-field-sized bytes behind an all-zero PathMeta
# direction -> (ingress ifindex, AS ingress interface ID or 0 for the internal link, egress interface ID)
DIRECTIONS = collections.OrderedDict((("ext", (1, 1, 2)), ("sib", (1, 1, 3)), ("ipfwd", (5, 0, 6)), ("int", (5, 0, 2))))
# BR 1's egress map (scion_hfv.topology): interface ID -> (kind, egress ifindex)
EGRESS = {1: ("link", 1), 2: ("link", 3), 3: ("sibling", 5), 4: ("sibling", 5), 5: ("sibling", 7), 6: ("sibling", 7)}
IP_ROUTE = {"ext": None, "sib": None, "ipfwd": 7, "int": None}     # fib_lookup_ip_forward on the frame's IP destination
FLIPS = ("seg_id", "ts", "exp", "cons_ingress", "cons_egress", "mac0", "mac1", "mac2", "mac3", "mac4", "mac5")
RULES = tuple(range(1, 10))


def path_offset(v6):
    """Offset of the PathMeta word: Ethernet, IPv4 or IPv6, UDP, SCION common and address header."""
    return 14 + (40 if v6 else 20) + 8 + 36


# ---- the model ----------------------------------------------------------------------------------

def seg_end_of(seg0, ci):
    """path_processing.h:84-86."""
    return seg0 * (min(ci, 2) + 1)


def geometry(seg0, num_inf, ci, ch):
    """(INF, HF, d, switch possible) from the integers alone.  A switch also needs CurrHF + 2 <= num_hf."""
    inf, hf = 4 + 8 * ci, 4 + 8 * num_inf + 12 * ch
    return inf, hf, inf - hf, ch + 1 == seg_end_of(seg0, ci)


def overlap_of(inf, hf, switch):
    """Which SegID store of the rewrite falls in bytes 1..11 of the checked hop field: (at INF+2, at INF+10)."""
    a, b = inf + 2, inf + 10
    return (a + 1 >= hf + 1 and a <= hf + 11, bool(switch) and b + 1 >= hf + 1 and b <= hf + 11)


def enumerate_overlaps():
    """{(store, d)} over seg0 0..63, num_inf 0..3, CurrINF 0..3, CurrHF 0..63 and both sides (from a
    neighbour AS, from the internal link), for frames that can reach the MAC check: from a neighbour
    CurrHF + 1 < num_hf for the largest num_hf the SegLens allow; a switch only from a neighbour.  Also
    returns whether INF+16 can end behind the switched hop field."""
    seen, bare = set(), False
    for seg0 in range(64):
        for ni in range(4):
            rest = ni - (seg0 > 0)
            if rest < 0 or rest > 2:
                continue
            max_hf = seg0 + 63 * rest
            for ci in range(4):
                for ch in range(64):
                    inf, hf, d, sw = geometry(seg0, ni, ci, ch)
                    if overlap_of(inf, hf, False)[0]:
                        seen.add(("int", "INF+2", d))
                    if ch + 1 >= max_hf:
                        continue                             # NOT_IMPLEMENTED before the MAC check
                    a, b = overlap_of(inf, hf, sw)
                    if a:
                        seen.add(("ext", "INF+2", d))
                    if b:
                        seen.add(("ext", "INF+10", d))
                    if sw and inf + 16 > hf + 24:
                        bare = True
    return seen, bare


class Walk:
    """What the walk of one frame gives (offsets relative to the PathMeta word)."""
    __slots__ = ("status", "verdict", "egress", "num_inf", "num_hf", "ci", "ch", "inf", "hf", "switch", "meta_out",
                 "stores", "mac", "d", "clob", "ifid_reads", "key_off", "out", "ci_out", "ch_out", "seg_end")


def _r16(p, o):
    return p[o] << 8 | p[o + 1]


def walk(path, plen, as_ing, ip_route=None, rule=0):
    """path: the frame from the PathMeta word on (bytes); plen: how many of them the frame has;
    as_ing: the AS interface ID the frame came in on, 0 for the internal link; ip_route: the egress
    ifindex of the frame's IP destination (None: no route).  Returns a Walk; .out is the path after the
    rewrite (the input where nothing is rewritten), .verdict the verdict before the MAC check
    (SCION_FORWARD standing for "rewritten, now check the MAC")."""
    w = Walk()
    w.out, w.switch, w.mac, w.stores, w.egress, w.d, w.clob = bytes(path), 0, None, [], -1, None, (False, False)
    w.ifid_reads, w.key_off, w.meta_out, w.inf, w.hf = [], None, None, None, None

    def end(status):
        w.status, w.verdict = status, V[status]
        return w

    if plen < 4:
        return end("PARSE_ERROR")
    meta = struct.unpack_from(">I", path, 0)[0]
    seg = ((meta >> 12) & 0x3F, (meta >> 6) & 0x3F, meta & 0x3F)
    ni = sum(1 for s in seg if s)
    if rule in (8, 9):
        ni = max([i + 1 for i in range(3) if seg[i]] or [0])
    nh = sum(seg)
    ci, ch = meta >> 30, (meta >> 24) & 0x3F
    w.num_inf, w.num_hf, w.ci, w.ch = ni, nh, ci, ch
    inf = 4 + 8 * ci
    w.inf = inf
    if inf + 8 > plen:
        return end("PARSE_ERROR")
    sid0, sid1 = _r16(path, inf + 2), 0
    if ci + 1 < ni:
        if inf + 16 > plen:
            return end("PARSE_ERROR")
        sid1 = _r16(path, inf + 10)
    elif rule == 6 and inf + 16 <= plen:
        sid1 = _r16(path, inf + 10)
    hf = 4 + 8 * ni + 12 * ch
    w.hf = hf
    if hf + 12 > plen:
        return end("PARSE_ERROR")
    if rule in (9, -1):                                      # the frame kernels' parse only
        return end("SCION_FORWARD")
    w.seg_end = seg_end_of(seg[0], ci)
    if rule == 1:
        w.seg_end = seg[0] + (seg[1] if ci >= 1 else 0) + (seg[2] if ci >= 2 else 0)
    if as_ing:
        c0 = path[inf] & 1
        f = hf + 2 if c0 else hf + 4
        w.ifid_reads.append(f)
        if _r16(path, f) != as_ing:
            return end("NO_INTERFACE")
        if path[hf] & 3:
            return end("ROUTER_ALERT")
        beta = sid0 ^ (0 if c0 else _r16(path, hf + 6))
        w.mac = (inf, hf, beta)
        if not c0:
            sid0 = beta
        nxt = ch + 1
        if rule != 7 and nxt >= nh:
            return end("NOT_IMPLEMENTED")
        if nxt == w.seg_end:
            w.switch, ci, ch, hf = 1, ci + 1, ch + 1, hf + 12
            if hf + 12 > plen:
                return end("PARSE_ERROR")
        if rule == 7 and nxt >= nh:
            return end("NOT_IMPLEMENTED")
    inf2 = inf + 8 * w.switch
    if w.switch and inf2 + 8 > plen:
        return end("ABORT")                                  # the bare return 0: never reached (enumerate_overlaps)
    w.key_off = hf + 4 if path[inf2] & 1 else hf + 2
    w.ifid_reads.append(w.key_off)
    kind, ifindex = EGRESS.get(_r16(path, w.key_off), (None, -1))
    if kind is None:
        return end("ABORT")
    if kind == "link":
        if path[hf] & 3:
            return end("ROUTER_ALERT")
        sid = sid1 if w.switch else sid0
        if not as_ing:
            w.mac = (inf, hf, sid)
        if path[inf2] & 1:
            sid ^= _r16(path, hf + 6)
        if w.switch:
            sid1 = sid
        else:
            sid0 = sid
        ch += 1
    elif not as_ing:
        if ip_route is None:
            return end("FIB_LKUP_PASS")
        ifindex = ip_route
    # rewrite_scion_path
    ci_st = min(ci, 3) if rule == 2 else ci
    ch_st = ch if rule == 3 else ch & 0x3F
    w.meta_out = ((meta & 0x00FFFFFF) | (ch_st << 24) | (ci_st << 30)) & 0xFFFFFFFF
    w.ci_out, w.ch_out = w.meta_out >> 30, (w.meta_out >> 24) & 0x3F
    out = bytearray(path)
    struct.pack_into(">I", out, 0, w.meta_out)
    w.stores.append((inf + 2, sid0))
    if w.switch and inf + 16 <= plen:
        w.stores.append((inf + 10, sid1))
    for off, val in w.stores:
        struct.pack_into(">H", out, off, val)
    w.out, w.egress = bytes(out), ifindex
    if w.mac:
        w.d = w.mac[0] - w.mac[1]
        w.clob = overlap_of(w.mac[0], w.mac[1], len(w.stores) > 1)
    return end("SCION_FORWARD")


def _tags(inputs):
    """The 6-byte MACs of macinput blocks under BR 1's key (checker-side AES-CMAC)."""
    hk, valid = orc.key_table(KEY)
    return orc.cmac16_bulk(np.frombuffer(b"".join(inputs), np.uint8).reshape(-1, 16), hk, valid)[:, :6]


def mac_fields(path, w, out=None, rule=0):
    """(macinput, MAC) of the walk's deferred check: from the bytes as they arrive, or (out given) as a
    kernel reads the hop field that looks after the rewrite: rule 4 plainly, rule 5 with the saved SegID
    bytes substituted two bytes too far.  The timestamp is never stored into."""
    inf, hf, beta = w.mac
    src = bytearray(path if out is None else out)
    if out is not None and rule == 5 and w.clob[0]:
        src[inf + 4:inf + 6] = path[inf + 2:inf + 4]
    ts = struct.unpack_from(">I", path, inf + 4)[0]
    return P.macinput(beta, ts, src[hf + 1], _r16(src, hf + 2), _r16(src, hf + 4)), bytes(src[hf + 6:hf + 12])


def mac_ok(path, w, after=False, rule=0):
    mi, mac = mac_fields(path, w, w.out if after else None, rule)
    return orc.cmac(mi, KEY)[:6] == mac


def judge(path, plen, as_ing, ip_route=None, hf_check=True, rule=0):
    """(verdict, egress ifindex, path after the router) by the model, MAC check included."""
    w = walk(path, plen, as_ing, ip_route, rule)
    if w.status != "SCION_FORWARD":
        return w.verdict, -1, w.out, w
    if hf_check and w.mac and not mac_ok(path, w, after=rule in (4, 5), rule=rule):
        return V["INVALID_HF"], w.egress, w.out, w
    return V["SCION_FORWARD"], w.egress, w.out, w


def locate(path, plen, rule=0):
    """(status, INF, HF) of frame_locate for a frame whose underlay and SCION header parse (rule 9: with
    num_inf taken as the index of the last non-zero SegLen plus one)."""
    w = walk(path, plen, 0, rule=9 if rule == 9 else -1)
    return (hfv.FRAME_PARSE_ERROR if w.status == "PARSE_ERROR" else 0), w.inf, w.hf


# ---- frames -------------------------------------------------------------------------------------

def encap(direction, v6):
    if DIRECTIONS[direction][1]:
        return TP.encaps(1, 2, v6)[0]
    _, internal = TP._addrs(v6)
    dst = internal["br3"][0] if direction == "ipfwd" else internal["br1"][0]
    return P.Encap(TP.MAC[4], TP.MAC[5], internal["br2"][0], dst, 31002, 31002)


def curr_hf_values(seg, ci):
    nh = sum(seg)
    true_end = sum(seg[:ci + 1]) if ci < 3 else nh
    vals = {0, 1, true_end - 1, nh - 2, nh - 1, nh, 62, 63}
    for se in (seg[0] * (ci + 1), seg_end_of(seg[0], ci)):
        vals |= {se - 2, se - 1, se}
    return sorted(x for x in vals if 0 <= x < 64)


def raw_path(seg, ci, ch, cons):
    """PathMeta, info fields (Cons bit s of `cons` for info field s) and filler hop fields."""
    ni, nh = sum(1 for s in seg if s), sum(seg)
    meta = (ci << 30) | (ch << 24) | (seg[0] << 12) | (seg[1] << 6) | seg[2]
    b = bytearray(struct.pack(">I", meta))
    for s in range(ni):
        b += struct.pack(">BBHI", (cons >> s) & 1, 0, 0x1111 * (s + 1) + 0x0204, 0x60000000 + 0x010203 * (s + 1))
    for t in range(nh or FILLER_HOPS):
        b += struct.pack(">BBHH", 0, 63 - t % 5, 4, 5) + bytes((17 * t + 29 * j + 1) & 0xFF for j in range(6))
    return b


def set_ifids(b, seg, ci, ch, direction):
    """The interface IDs of the hop field(s) the router reads, for the Cons bits that govern them."""
    _, as_ing, egr = DIRECTIONS[direction]
    ni, nh = sum(1 for s in seg if s), sum(seg)
    inf, hf, _, sw = geometry(seg[0], ni, ci, ch)
    sw = bool(as_ing) and sw and ch + 1 < nh
    for _ in range(2):                                       # a second pass where the first changed a Cons bit
        if hf + 12 > len(b) or inf + 8 > len(b):
            return
        c0 = b[inf] & 1
        if as_ing:
            struct.pack_into(">H", b, hf + 2 if c0 else hf + 4, as_ing)
        hf2, inf2 = hf + 12 * sw, inf + 8 * sw
        if hf2 + 12 > len(b) or inf2 + 8 > len(b):
            return
        c1 = b[inf2] & 1
        if sw or not as_ing:
            struct.pack_into(">H", b, hf2 + 2 if c1 else hf2 + 4, 0 if sw else 9)
        struct.pack_into(">H", b, hf2 + 4 if c1 else hf2 + 2, egr)


class Item:
    """One frame of the corpus before it is laid into its slot."""
    __slots__ = ("kind", "what", "layout", "ci", "ch", "cons", "direction", "path", "cut", "base", "payload")

    def __init__(self, kind, what, layout, ci, ch, cons, direction, path, cut=None, base=-1, payload=True):
        self.kind, self.what, self.layout, self.ci, self.ch, self.cons = kind, what, layout, ci, ch, cons
        self.direction, self.path, self.cut, self.base, self.payload = direction, bytes(path), cut, base, payload


def _walk_of(b, direction, plen=None):
    _, as_ing, _ = DIRECTIONS[direction]
    return walk(bytes(b) + P.PAYLOAD, (len(b) + len(P.PAYLOAD)) if plen is None else plen, as_ing, IP_ROUTE[direction])


def is_case_a(w):
    if w.status != "SCION_FORWARD" or not w.mac:
        return False
    inf, hf, _ = w.mac
    return inf + 8 <= hf or inf + 2 >= hf + 12


def flip_twin(b, w, direction, what, k):
    """The case-A path with one bit of field `what` flipped (k picks the bit), or None where that field
    must stay (an interface ID the walk reads, other than bit 0 of the egress key 2 <-> 3 of a frame from
    a neighbour AS)."""
    inf, hf, _ = w.mac
    t = bytearray(b)
    if what == "seg_id":
        t[inf + 2 + k % 2] ^= 1 << (k // 2 % 8)
    elif what == "ts":
        t[inf + 4 + k % 4] ^= 1 << (k // 4 % 8)
    elif what == "exp":
        t[hf + 1] ^= 1 << (k % 8)
    elif what in ("cons_ingress", "cons_egress"):
        f = hf + (2 if what == "cons_ingress" else 4)
        if f not in w.ifid_reads:
            t[f + k % 2] ^= 1 << (k // 2 % 8)
        elif f == w.key_off and DIRECTIONS[direction][1] and not w.switch:
            t[f + 1] ^= 1
        else:
            return None
    else:
        t[hf + 6 + int(what[3])] ^= 1 << (k % 8)
    return t


# ---- the overlap class --------------------------------------------------------------------------
# CurrINF past the info field of a one-segment path [3], from AS interface 1 to 2: the "info field" lies
# in the hop fields and the rewrite's SegID store at INF+2 falls into the hop field under check.
#   d8       CurrINF 2, CurrHF 0: INF = HF + 8.  Cons is bit 0 of MAC[2], the SegID MAC[4:6], the
#            timestamp bytes 0..3 of the next hop field.  Valid as it arrives (br_fuzz.OVERLAP_MAC);
#            scion_as_egress then stores beta ^ MAC[0:2] into MAC[4:6].
#   d8_after MAC[4:6] = SegID with tag[4:6] ^ tag[0:2] == SegID: wrong as it arrives, equal to the tag
#            once the rewrite has stored the new SegID.  INVALID_HF by the reference.
#   d0       CurrINF 1, CurrHF 0: INF = HF.  Flags 0 so Cons 0; SegID = ConsIngress = the egress
#            interface, ConsEgress = the ingress interface, timestamp = ConsEgress | MAC[0:2], beta =
#            ConsIngress ^ MAC[0:2]: a 16-bit fixed point tag[0:2] == MAC[0:2].
#   d0_after the same with ConsIngress replaced by beta in the MAC input: valid only after the rewrite.
#   d4       CurrINF 3, CurrHF 1: INF = HF + 4, SegID = MAC[0:2], timestamp = MAC[2:6].  A passing MAC
#            would need a 2^32 search: failing frames only; the store zeroes MAC[0:2].
# Each constant is (free byte, MAC): the free byte is the next hop field's ConsIngress (d8) or the
# ExpTime (d0).  search_overlap() finds them (one 2^16 sweep per free byte value); the CPU test
# re-checks them.
OVERLAP = {
    "d8": ((5, "a2632378128d"),),
    "d8_after": ((11, "b3cb5930515f"), (13, "d1fcb9859c43")),
    "d0": ((63, "57f99d6fc0c4"), (63, "9c093cfa6500")),
    "d0_after": ((63, "1b36a99bf336"), (63, "acbc89b46654")),
}
OVERLAP_D4_MACS = ("0102030405a6", "ffee00112233", "000000000000")


def overlap_path(kind, free, mac):
    mac = bytes.fromhex(mac) if isinstance(mac, str) else bytes(mac)
    info = P.InfoField(True, seg_id=0x4242, ts=0x61000000).pack()
    if kind.startswith("d8"):
        hops = [P.HopField(1, 2, exp=63, mac=mac), P.HopField(free, 7, exp=63), P.HopField(3, 4)]
        ci, ch = 2, 0
    elif kind.startswith("d0"):
        hops = [P.HopField(2, 1, exp=free, mac=mac), P.HopField(5, 7, exp=63), P.HopField(3, 4)]
        ci, ch = 1, 0
    else:
        hops = [P.HopField(3, 4), P.HopField(2, 1, exp=63, mac=mac), P.HopField(5, 7, exp=63)]
        ci, ch = 3, 1
    return struct.pack(">I", (ci << 30) | (ch << 24) | (3 << 12)) + info + b"".join(h.pack() for h in hops), ci, ch


def search_overlap(kind, free_values=range(1, 64), want=1):
    """[(free byte, MAC hex)]: one 2^16 sweep per free byte value until `want` are found."""
    found = []
    x = np.arange(65536)
    for free in free_values:
        if kind.startswith("d8"):          # x: the SegID as it arrives (= beta, Cons 1)
            mi = [P.macinput(v, (63 << 16) | free, 63, 1, 2) for v in x]
            tags = _tags(mi).astype(np.int64)
            t01, t45 = tags[:, 0] << 8 | tags[:, 1], tags[:, 4] << 8 | tags[:, 5]
            if kind == "d8":
                hit = (t45 == x) & (tags[:, 2] & 1 == 1)
                macs = [bytes(tags[i].astype(np.uint8)) for i in np.nonzero(hit)[0]]
            else:
                hit = ((t45 ^ t01) == x) & (tags[:, 2] & 1 == 1) & (t01 != 0)
                macs = [bytes(tags[i, :4].astype(np.uint8)) + struct.pack(">H", int(x[i])) for i in np.nonzero(hit)[0]]
        else:                               # x: MAC[0:2]; beta = ConsIngress ^ x, timestamp = ConsEgress | x
            ing = (x ^ 2) if kind == "d0_after" else np.full(65536, 2)
            mi = [P.macinput(int(v) ^ 2, (1 << 16) | int(v), free, int(g), 1) for v, g in zip(x, ing)]
            tags = _tags(mi).astype(np.int64)
            hit = (tags[:, 0] << 8 | tags[:, 1]) == x
            macs = [bytes(tags[i].astype(np.uint8)) for i in np.nonzero(hit)[0]]
        found += [(free, m.hex()) for m in macs]
        if len(found) >= want:
            break
    return found


# ---- the corpus ---------------------------------------------------------------------------------

def _base_items():
    items = []
    for seg in LAYOUTS:
        ni = sum(1 for s in seg if s)
        for ci in range(4):
            for ch in curr_hf_values(seg, ci):
                for cons in range(1 << ni):
                    for direction in DIRECTIONS:
                        b = raw_path(seg, ci, ch, cons)
                        set_ifids(b, seg, ci, ch, direction)
                        w = _walk_of(b, direction)
                        if is_case_a(w):
                            _make_valid(b, w, direction)
                            w = _walk_of(b, direction)
                            assert is_case_a(w)
                        items.append(Item("base", "A" if is_case_a(w) else "", seg, ci, ch, cons, direction, b))
    return items


def _make_valid(b, w, direction):
    inf, hf, _ = w.mac
    ts = struct.unpack_from(">I", b, inf + 4)[0]
    beta = _r16(b, inf + 2)
    mac = orc.cmac(P.macinput(beta, ts, b[hf + 1], _r16(b, hf + 2), _r16(b, hf + 4)), KEY)[:6]
    b[hf + 6:hf + 12] = mac
    if DIRECTIONS[direction][1] and not (b[inf] & 1):        # Cons 0 at ingress: beta = SegID ^ MAC[0:2]
        struct.pack_into(">H", b, inf + 2, beta ^ _r16(mac, 0))


@functools.lru_cache(maxsize=None)
def items():
    """The corpus as Items, the same for both families.  Read-only."""
    out = _base_items()
    n_base = len(out)
    k = 0
    for i in range(n_base):
        it = out[i]
        if it.what != "A":
            continue
        b = bytearray(it.path)
        w = _walk_of(b, it.direction)
        made = 0
        while made < 2:
            what = FLIPS[k % len(FLIPS)]
            t = flip_twin(b, w, it.direction, what, k // len(FLIPS))
            k += 1
            if t is None:
                continue
            out.append(Item("flip", what, it.layout, it.ci, it.ch, it.cons, it.direction, t, base=i))
            made += 1
        t = bytearray(b)
        inf, hf, _ = w.mac
        if it.ci < w.num_inf and i % 2:
            t[inf + 1] ^= 1 << (i % 8)
            what = "inf1"
        else:
            t[hf] ^= 4 << (i % 6)
            what = "hf0"
        out.append(Item("dontcare", what, it.layout, it.ci, it.ch, it.cons, it.direction, t, base=i))
    for i in range(n_base):                                  # router alert flags on the hop field each side reads
        it = out[i]
        if it.what != "A":
            continue
        w = _walk_of(it.path, it.direction)
        what, off = ("hf_switched", w.hf + 12) if w.switch and i % 2 else ("hf", w.hf)
        t = bytearray(it.path)
        t[off] |= 1 + i % 3
        out.append(Item("alert", what, it.layout, it.ci, it.ch, it.cons, it.direction, t, base=i))
    for i in range(n_base):                                  # CurrHF + 1 == num_hf == seg_end, without payload
        it = out[i]
        nh = sum(it.layout)
        if DIRECTIONS[it.direction][1] and it.ch + 1 == nh == seg_end_of(it.layout[0], it.ci):
            out.append(Item("short", "", it.layout, it.ci, it.ch, it.cons, it.direction, it.path, base=i, payload=False))
    first_overlap = {}
    for kind in ("d8", "d8_after", "d0", "d0_after"):
        for free, mac in OVERLAP[kind]:
            p, ci, ch = overlap_path(kind, free, mac)
            first_overlap.setdefault(kind, len(out))
            out.append(Item("overlap", kind, (3, 0, 0), ci, ch, 1, "ext", p))
    for mac in OVERLAP_D4_MACS:
        p, ci, ch = overlap_path("d4", 0, mac)
        first_overlap.setdefault("d4", len(out))
        out.append(Item("overlap", "d4", (3, 0, 0), ci, ch, 1, "ext", p))
    # truncations: the first (shallowest) forwarding frame of each switch kind, and one per overlap kind
    picks = {}
    for i in range(n_base):
        it = out[i]
        if it.what != "A" or it.direction != "ext":
            continue
        w = _walk_of(it.path, it.direction)
        if not w.switch:
            continue
        real = it.ci < w.num_inf
        name = "ci%d%s%s" % (it.ci, "" if it.ci + 1 < w.num_inf else "_unparsed", "" if real else "_pastinf")
        if name not in picks or w.hf < picks[name][1]:
            picks[name] = (i, w.hf)
    for name, i in sorted([(n, i) for n, (i, _) in picks.items()] + [("overlap_" + k, i) for k, i in first_overlap.items()]):
        it = out[i]
        w = _walk_of(it.path, it.direction)
        for cut in range(0, min(w.hf + 24, len(it.path) + len(P.PAYLOAD)) + 1):
            out.append(Item("trunc", name, it.layout, it.ci, it.ch, it.cons, it.direction, it.path, cut=cut, base=i))
    return tuple(out)


class Corpus:
    """frames u8[n, 1024], lens u16[n], ifidx u32[n] of one family, with the Items beside them."""

    def __init__(self, v6):
        its = items()
        self.v6, self.items, self.n, self.P = v6, its, len(its), path_offset(v6)
        self.cfg = TP.br_config("br1", v6)
        self.frames = np.zeros((self.n, SLOT), np.uint8)
        self.lens = np.zeros(self.n, np.uint16)
        self.ifidx = np.array([DIRECTIONS[it.direction][0] for it in its], np.uint32)
        encs = {d: encap(d, v6) for d in DIRECTIONS}
        for i, it in enumerate(its):
            f = encs[it.direction].frame(P.scion_header(it.path, payload=P.PAYLOAD if it.payload else b""))
            assert len(f) <= SLOT and len(it.path) // 4 + 9 < 256
            self.frames[i, :len(f)] = np.frombuffer(f, np.uint8)
            self.lens[i] = len(f) if it.cut is None else self.P + it.cut
        self.kind = np.array([it.kind for it in its])
        self.what = np.array([it.what for it in its])
        self.direction = np.array([it.direction for it in its])
        self.internal = self.ifidx == 5
        for a in (self.frames, self.lens, self.ifidx):
            a.setflags(write=False)

    def path(self, i):
        """(path bytes as the frame holds them, bytes of them present) of frame i."""
        return self.frames[i, self.P:].tobytes(), int(self.lens[i]) - self.P

    def walk(self, i, rule=0):
        it = self.items[i]
        p, plen = self.path(i)
        return walk(p, plen, DIRECTIONS[it.direction][1], IP_ROUTE[it.direction], rule)

    def judge(self, i, hf_check=True, rule=0):
        it = self.items[i]
        p, plen = self.path(i)
        return judge(p, plen, DIRECTIONS[it.direction][1], IP_ROUTE[it.direction], hf_check, rule)


@functools.lru_cache(maxsize=None)
def corpus(v6):
    return Corpus(bool(v6))


@functools.lru_cache(maxsize=None)
def expected(v6, hf_check=True, key=True):
    """((action, verdict, egress, stats), frames out) of the CPU checker over corpus(v6).  Read-only."""
    c = corpus(v6)
    out = c.frames.copy()
    res = orc.br_process(out, c.lens, c.ifidx, c.cfg, HK if key else None, hf_check=hf_check)
    for a in res + (out,):
        a.setflags(write=False)
    return res, out


def orders(v6):
    """The two orders the GPU legs run the corpus in: shuffled with a fixed seed, so that every 64-frame
    tile mixes kinds, and sorted by (verdict, direction, kind, switch), so that whole tiles take one
    branch of the walk."""
    c = corpus(v6)
    (_, verdict, _, _), _ = expected(v6)
    sw = np.array([c.walk(i).switch for i in range(c.n)])
    return {"shuffled": np.random.default_rng(20260).permutation(c.n),
            "sorted": np.lexsort((sw, c.kind, c.direction, verdict))}


# ---- the placement table ------------------------------------------------------------------------

def placement(v6):
    """One record per frame, from the checker's results (verdict, the PathMeta word it stored) and the
    model's walk: (verdict, CurrINF in, CurrINF stored, CurrHF stored - CurrHF in, switch, overlap d or
    None, MAC valid before the rewrite, after it, direction), None where no MAC is checked, and the
    frame's names in ROWS."""
    c = corpus(v6)
    (_, verdict, _, _), out = expected(v6)
    recs = []
    for i, it in enumerate(c.items):
        p, plen = c.path(i)
        w = c.walk(i)
        v = int(verdict[i])
        names = []
        key = (v, w.ci if plen >= 4 else None, None, None, w.switch, None, None, None, it.direction)
        rewritten = w.status == "SCION_FORWARD"
        if rewritten:
            m = struct.unpack_from(">I", out[i], c.P)[0]
            before = mac_ok(p, w) if w.mac else None
            after = mac_ok(p, w, after=True, rule=4) if w.mac else None
            d = w.d if w.mac and any(w.clob) else None
            key = (v, w.ci, m >> 30, ((m >> 24) & 0x3F) - w.ch, w.switch, d, before, after, it.direction)
        seg = it.layout
        real = plen >= 4 and w.ci < w.num_inf
        true_end = sum(seg[:w.ci + 1]) if real else None
        fwd = v == V["SCION_FORWARD"]
        ext = bool(DIRECTIONS[it.direction][1])
        if fwd and w.switch:
            names.append("switch_ci%d" % w.ci)
            if w.ci == 3 and key[2] == 0:
                names.append("switch_ci3_stored_0")
            if w.ch == 62 and key[3] == -62:
                names.append("hf62_to_0_switch")
            if real and w.ch + 1 != true_end and key[6]:
                names.append("switch_inside_real_segment")
            if w.ci + 1 >= w.num_inf and len(w.stores) == 2 and w.stores[1][0] >= 4 + 8 * w.num_inf:
                names.append("switch_seg_id1_unparsed")
        if fwd and not w.switch:
            if w.ch == 63 and key[3] == -63:
                names.append("hf63_to_0")
            if ext and real and w.ch + 1 == true_end and w.ch + 1 < w.num_hf and key[6]:
                names.append("no_switch_at_real_end")
            if ext and seg[0] == 0 and w.num_hf:
                names.append("seg0_zero_forward")
        if v == V["NOT_IMPLEMENTED"] and w.status == "NOT_IMPLEMENTED":
            names.append("not_implemented")
            if w.ch + 1 == w.num_hf == w.seg_end:
                names.append("not_implemented_at_seg_end")
        if it.kind == "overlap":
            names.append("overlap_%s_%s" % (it.what, "forward" if fwd else "invalid_hf" if v == V["INVALID_HF"] else v))
        if v == V["ROUTER_ALERT"]:
            names.append("alert_%s_ci%d" % ("egress" if it.what == "hf_switched" or not ext else "ingress", w.ci))
        if it.kind == "trunc":
            if v == V["PARSE_ERROR"]:
                names.append("trunc_parse" if w.hf is None or w.hf + 12 > plen else "trunc_switched_hf")
            else:
                names.append("trunc_whole")
        recs.append((key, tuple(names)))
    return recs


# How many frames of the corpus (either family) carry each name of placement().
ROWS = {
    # a forwarding segment switch at each CurrINF; CurrINF 3 -> 4 is stored as 0
    "switch_ci0": 281, "switch_ci1": 182, "switch_ci2": 41, "switch_ci3": 41, "switch_ci3_stored_0": 41,
    # CurrHF 63 -> 64 stored as 0, and 62 -> 64 through a switch
    "hf63_to_0": 96, "hf62_to_0_switch": 8,
    # seg_end = seg0 * k: a switch inside a real segment, none at a real segment end (valid MAC, forwarded)
    "switch_inside_real_segment": 61, "no_switch_at_real_end": 48,
    # CurrINF + 1 >= num_inf at a switch: seg_id1 was never parsed, its store lands in the hop fields
    "switch_seg_id1_unparsed": 143,
    "seg0_zero_forward": 32,
    "not_implemented": 572, "not_implemented_at_seg_end": 216,
    "overlap_d8_forward": 1, "overlap_d8_after_invalid_hf": 2, "overlap_d0_forward": 2, "overlap_d0_after_invalid_hf": 2,
    "overlap_d4_invalid_hf": 3,
    "alert_ingress_ci0": 432, "alert_ingress_ci1": 404, "alert_ingress_ci2": 288, "alert_ingress_ci3": 192,
    "alert_egress_ci0": 301, "alert_egress_ci1": 276, "alert_egress_ci2": 205, "alert_egress_ci3": 158,
    # cut frames: PARSE_ERROR from the parse, PARSE_ERROR from the switched hop field, long enough to be whole
    "trunc_parse": 380, "trunc_switched_hf": 60, "trunc_whole": 62,
}
N_FRAMES = 17580
FIXTURE_WIDTH = 160               # every byte the router changes lies below: underlay, PathMeta, INF+2.. INF+11 <= path + 40
