"""The checksum-edge corpus of tests/br_csum.py on the CPU: where its frames land (asserted cell by
cell: checksum kind x next-hop kind x class of D), that every wrong rule of br_csum.VARIANTS
changes a check field of the corpus for every checksum kind, that the plain-integer model gives the
oracle's two check fields on every frame, that the oracle equals the reference's own program where
it is built, and tests/golden/br_csum.npz (what the reference program gave) everywhere.  Integer
work: every comparison is exact.

What the fuzz reaches (test_fuzz_parity_batches_recounted counts it again, without asserting the
misses): of the 72,308 frames the six 20000-frame batches of test_gpu_br.test_fuzz_parity forward
(br1/br2/br3, IPv4 seed 100 and IPv6 seed 101), frames with a check field in the class:

    D < 0, |D| < 2^16    8795        D > 0, |D| < 2^16      958
    D < 0, |D| < 2^32   19630        D > 0, |D| < 2^32    43883
    D = 0, |D| >= 2^32, D > 0 with D = 0 mod 65535, bit 16 after fold 2, two folds != full
    fold, a result of 0x0000 / 0xffff / 0x0001 / 0xfffe, an incoming field of 0x0000 / 0xffff:  0

so of the wrong rules only 3 (~C at 16 bits: every frame) and 4 (cs cut to 32 bits: every frame with
D < 0, 28425) change a frame of those batches; 1 (a third fold), 2 (zero test on the low half) and
5 (RFC 1624) change none of them.
"""
import numpy as np
import pytest

import br_csum as C
import br_topo as T
import orc

HK = orc.hop_key(T.KEYS[1])
needs_ref = pytest.mark.skipif(not orc.ref_br_available(), reason="reference router not built (oracle/_ref)")
LEG_SIZES = {"v4_base": 90, "v4_mid": 35, "v4_hi": 13, "v4_lo": 14, "v6_base": 68, "v6_hi": 10, "v6_lo": 2}

U = None    # unreachable: no (R, C) within the next-hop kind's bound on R is in the class
# (checksum kind, next-hop kind) -> frames per class, in the order of br_csum.CLASS_NAMES:
#   D = 0 | D < 0: < 2^16, < 2^32, >= 2^32 | D > 0: < 2^16, < 2^32, >= 2^32 | D > 0, = 0 mod 65535 |
#   D > 0, bit 16 after fold 2 | D < 0, result 0 | two folds != full fold |
#   result 0x0000, 0xffff, 0x0001, 0xfffe | C 0x0000, 0xffff
PLACEMENT = {
    ("ip4", "link"): (2, 12, 7, 8, 13, 9, 7, 2, 1, 2, 6, 4, 4, 5, 3, 4, 4),
    ("ip4", "sibling"): (2, 8, 9, 7, 9, 13, 6, 2, 1, 2, 6, 4, 4, 5, 3, 3, 4),
    ("ip4", "ipfwd"): (1, 33, 3, U, 3, U, U, U, U, U, U, U, 2, 9, 2, 8, 4),
    ("udp4", "link"): (2, 7, 9, 7, 13, 12, 8, 2, 3, 2, 8, 4, 5, 5, 4, 4, 4),
    ("udp4", "sibling"): (2, 11, 14, 8, 6, 7, 6, 2, 1, 2, 6, 4, 4, 5, 3, 3, 4),
    ("udp4", "ipfwd"): (8, 32, U, U, U, U, U, U, U, U, U, U, 10, 1, 1, 8, 2),
    ("udp6", "link"): (2, 5, 4, 5, 5, 5, 5, 2, 3, 2, 9, 4, 5, 6, 4, 4, 4),
    ("udp6", "sibling"): (2, 5, 4, 5, 5, 5, 5, 2, 3, 2, 9, 4, 5, 6, 4, 4, 4),
    ("udp6", "ipfwd"): (8, 10, U, U, U, U, U, U, U, U, U, U, 10, 1, 1, 8, 2),
}
# An IP forward is taken only by a frame from an internal interface (as_ing_ifid 0) whose egress
# entry is a sibling's: neither as_ingress nor as_egress ran, so PathMeta and the SegIDs are stored
# as they came, and fib_ip_forward keeps addresses and ports.  What is left is the IPv4 TTL: one
# less, or 255 for 0.
IPFWD_R = {"ip4": (-1, 255), "udp4": (0,), "udp6": (0,)}


# Two IPv4 addresses change R by less than 2^33 either way, and the "hi" tables' link addresses (a tag
# byte below 0xff each) and ingress address keep the header's R below 0x1ffffffff; the UDP checksum's
# R also has the two new ports and reaches 0x20000ffff.
BEYOND_IPV4 = {"negative, one off, second": ("ip4", "udp4"), "bit 16, f1 >> 16 = 2, above 2^33": ("ip4",),
               "bit 16, f1 >> 16 = 2, below 2^33": ("ip4",)}


def each_frame():
    for name, v6, table, cfg, frames, lens, ifidx, meta in C.legs():
        out = C.oracle(name)[1]
        for i in range(len(frames)):
            yield name, cfg, bytes(frames[i, :lens[i]]), bytes(out[i, :lens[i]]), meta[i]


# ---- coverage, as asserted conditions -----------------------------------------------------------

def test_every_corpus_frame_is_forwarded():
    total = 0
    for name, v6, table, cfg, frames, lens, ifidx, meta in C.legs():
        (a, v, e, _), out = C.oracle(name)
        assert len(frames) == LEG_SIZES[name] == len(meta) and frames.shape[1] == 256, name
        assert (a == 4).all() and (v == C.FORWARD).all(), name
        assert (out != frames).any(axis=1).all()
        total += len(frames)
    assert total == sum(LEG_SIZES.values()) == 232          # well under 1024 frames of 256 bytes


def test_frames_land_where_they_were_aimed():
    """The checksum a frame was solved for has exactly the D it was solved for, and the next hop it
    was built for; every edge target has a frame on a link for every checksum kind."""
    aimed = set()
    for name, cfg, fin, fout, (target, nh, pkind, kind, D) in each_frame():
        R, c = C.residuals(fin, fout)[kind]
        assert D is None or R - c == D, (name, target, nh, kind)
        assert C.next_hop_kind(cfg, fin, fout) == nh
        aimed.add((target, nh, kind))
    for target in C.EDGE_TARGETS:
        for kind in C.KINDS:
            assert ((target, "link", kind) in aimed) == (kind not in BEYOND_IPV4.get(target, ())), (target, kind)


def test_placement_table():
    table = C.placement()
    for (kind, nh), row in PLACEMENT.items():
        assert len(row) == len(C.CLASS_NAMES)
        for cls, n in zip(C.CLASS_NAMES, row):
            assert table[(kind, nh, cls)] == (n or 0), (kind, nh, cls)
            assert n is None or n > 0                      # every cell is non-empty or marked unreachable
            assert n is not None or nh == "ipfwd"          # and only an IP forward has unreachable cells
    assert set(PLACEMENT) == {(k, h) for k in C.KINDS for h in C.NEXT_HOPS}


def test_unreachable_cells_follow_from_the_bound_on_r():
    """Every IP forward of the corpus has R inside IPFWD_R, and a cell is marked unreachable exactly
    where no R of that set and no incoming field 0..0xffff is in the class."""
    seen = {k: set() for k in C.KINDS}
    for name, cfg, fin, fout, meta in each_frame():
        if C.next_hop_kind(cfg, fin, fout) == "ipfwd":
            for kind, (R, _) in C.residuals(fin, fout).items():
                seen[kind].add(R)
    for kind in C.KINDS:
        assert seen[kind] == set(IPFWD_R[kind]), kind
        reach = set()
        for R in IPFWD_R[kind]:
            for c in range(0x10000):
                reach.update(C.classes_of(R, c))
        marked = {cls for cls, n in zip(C.CLASS_NAMES, PLACEMENT[(kind, "ipfwd")]) if n is None}
        assert marked == set(C.CLASS_NAMES) - reach, kind


def test_bit_16_and_second_segid_and_ttl_coverage():
    f1hi = {k: set() for k in C.KINDS}
    seg1_edge, ttls = 0, {k: set() for k in C.KINDS}
    for name, cfg, fin, fout, (target, nh, pkind, kind, D) in each_frame():
        v6, _, fields = C.layout(fin)
        for k, (R, c) in C.residuals(fin, fout).items():
            cl = C.classify(R, c)
            if cl["bit16"]:
                f1hi[k].add(cl["f1hi"])
        if nh == "ipfwd":
            ttls[kind].add(fin[21 if v6 else 22])
        off, size = fields[kind][-1]
        if pkind == "seg_switch" and nh != "ipfwd" and target in C.EDGE_TARGETS and kind != "ip4":
            assert size == 2 and C.S.field_offsets(fin)["seg1"] == (off, size)
            seg1_edge += fin[off:off + 2] != fout[off:off + 2]       # the second SegID is part of this R
    # f1 >> 16 = 2 with bit 16 left needs D >= 0x1ffffffff: past the IPv4 header's R (BEYOND_IPV4)
    assert f1hi == {"ip4": {1}, "udp4": {1, 2}, "udp6": {1, 2}}
    assert seg1_edge >= 8
    for kind in C.KINDS:
        assert ttls[kind] >= set(C.TTLS), kind


def test_every_wrong_rule_changes_a_corpus_frame():
    changed = {(v, k): 0 for v in C.VARIANTS for k in C.KINDS}
    for name, cfg, fin, fout, meta in each_frame():
        for kind, (R, c) in C.residuals(fin, fout).items():
            for v in C.VARIANTS:
                changed[(v, kind)] += C.rule(R, c, v)[3] != C.rule(R, c)[3]
    for key, n in changed.items():
        assert n >= 4, (C.VARIANT_NAMES[key[0]], key[1])


def test_rule_examples():
    """The rule at the values the module's text names."""
    for D, res, ordinary in ((65535, 0x0000, 0xFFFF), (0x1FFFE0001, 0xFFFF, 0xFFFE), (-8014733896, 0x0000, 0x0001),
                             (-28182868007, 0x0001, 0x0002), (0, 0xFFFF, 0xFFFF), (-1, 0x0001, 0x0001)):
        assert C.rule(D, 0)[3] == C.rule(D + 0x1234, 0x1234)[3] == res and C.full(D) == ordinary, D
    assert C.rule(C.NEG_ZERO, 0)[3] == 0 and -(1 << 33) == C.NEG_ONE_OFF < C.NEG_ZERO < -(1 << 32)
    assert (C.rule(C.NEG_ONE_OFF, 0)[3], C.full(C.NEG_ONE_OFF)) == (0x0001, 0x0002)
    for m in list(range(1, 70000, 7)) + list(range((1 << 32) - 70000, 1 << 32, 3)):   # -2^32 < D < 0: never off
        assert C.rule(-m, 0)[3] == C.full(-m)


# ---- judges -------------------------------------------------------------------------------------

def test_model_against_the_oracle():
    for name, cfg, fin, fout, meta in each_frame():
        _, checks, _ = C.layout(fin)
        for kind, (R, c) in C.residuals(fin, fout).items():
            assert C.le(fout, checks[kind], 2) == C.rule(R, c)[3], (name, meta, kind)


@needs_ref
def test_oracle_against_the_reference_program():
    for name, v6, table, cfg, frames, lens, ifidx, _ in C.legs():
        res, out = C.oracle(name)
        prog = frames.copy()
        orc.assert_br_equal(res, out, orc.ref_br_process(prog, lens, ifidx, cfg, HK), prog, name)


def test_fixture_holds_the_corpus():
    g = orc.load_golden("br_csum.npz")
    legs = C.fixture_legs(g)
    assert [leg[0] for leg in legs] == [leg[0] for leg in C.legs()]
    for (name, cfg, frames, lens, ifidx, _, _), mine in zip(legs, C.legs()):
        assert bytes(cfg) == bytes(mine[3]), "the generator drifted: tables of " + name
        assert all(np.array_equal(a, b) for a, b in zip((frames, lens, ifidx), mine[4:7])), "the generator drifted: " + name


def test_oracle_reproduces_the_fixture():
    """tests/golden/br_csum.npz: what the reference program gave (make_golden.py br_csum), on the
    fixture's own frames and tables.  Needs no reference build."""
    for name, cfg, frames, lens, ifidx, want, want_frames in C.fixture_legs(orc.load_golden("br_csum.npz")):
        out = frames.copy()
        orc.assert_br_equal(orc.br_process(out, lens, ifidx, cfg, HK), out, want, want_frames, name)


@needs_ref
def test_reference_program_reproduces_the_fixture():
    for name, cfg, frames, lens, ifidx, want, want_frames in C.fixture_legs(orc.load_golden("br_csum.npz")):
        prog = frames.copy()
        orc.assert_br_equal(orc.ref_br_process(prog, lens, ifidx, cfg, HK), prog, want, want_frames, name)


# ---- what the fuzz reaches ----------------------------------------------------------------------

def test_fuzz_parity_batches_recounted(capsys):
    """The model over the frames the six test_fuzz_parity batches forward: it gives the oracle's
    check fields on every one.  The class counts are printed, not asserted (module docstring)."""
    total, counts, variants = 0, {c: 0 for c in C.CLASS_NAMES}, {v: 0 for v in C.VARIANTS}
    for br, v6 in C.FUZZ_BATCHES:
        n, cnt, wrong, var = C.fuzz_recount(br, v6)
        assert n > 0 and wrong == 0, (br, v6)
        total += n
        for c in cnt:
            counts[c] += cnt[c]
        for v in var:
            variants[v] += var[v]
    with capsys.disabled():
        print("\nfuzz_parity batches: %d forwarded frames; per class %s; changed by wrong rule %s" % (total, counts, variants))
