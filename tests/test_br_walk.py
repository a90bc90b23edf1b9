"""tests/br_walk.py held to itself, to the CPU checker, to the reference program and to the host parser
(no GPU): what the enumeration of the path-walk space shows, the searched overlap constants, the
placement table of the corpus with its counts, the case-A frames and their twins, the checker against
the model, against the reference program where it is built and against tests/golden/br_walk.npz
everywhere, the wrong rules of `make pathwalk` restated in the model (each changes a verdict or an
output byte of the corpus), and hfv_frame_locate / hfv_frame_extract against the model's offsets."""
import collections
import struct

import numpy as np
import pytest

import br_shift as S
import br_walk as W
import frames_rx_ref as R
import orc
import scion_hfv as hfv

V = hfv.VERDICT
FAMILIES = [False, True]
FAM_IDS = ["ipv4", "ipv6"]


# ---- the model ----------------------------------------------------------------------------------

def test_which_overlaps_can_occur():
    """Over seg0 0..63, num_inf 0..3, CurrINF 0..3, CurrHF 0..63: only the SegID store at INF+2 can fall
    in the checked hop field, at d = INF - HF in {0, 4, 8}, from either side; the store at INF+10 never
    does on a frame that reaches the MAC check (`clob & 2` of keep_mac_bytes is defensive only); and
    the bare `return 0` after a switch is out of reach."""
    seen, bare = W.enumerate_overlaps()
    assert seen == {(side, "INF+2", d) for side in ("ext", "int") for d in (0, 4, 8)}
    assert not bare


def test_seg_end_literals():
    assert [W.seg_end_of(2, ci) for ci in range(4)] == [2, 4, 6, 6]      # the reference adds seg0 twice at the most
    assert W.geometry(2, 2, 1, 3) == (12, 56, -44, True)                 # [2,3,0] at CurrINF 1, CurrHF 3: a switch
    assert W.geometry(2, 2, 1, 4)[3] is False                            # and none at the segment's true end
    assert W.geometry(3, 1, 2, 0)[2] == 8 and W.geometry(3, 1, 1, 0)[2] == 0 and W.geometry(3, 1, 3, 1)[2] == 4
    assert W.overlap_of(20, 12, 0) == (True, False) and W.overlap_of(12, 12, 0) == (True, False)
    assert W.overlap_of(4, 12, 1) == (False, True) and W.overlap_of(4, 24, 1) == (False, False)
    assert W.curr_hf_values((2, 3, 0), 1) == [0, 1, 2, 3, 4, 5, 62, 63]
    assert W.path_offset(False) == 78 and W.path_offset(True) == 98


def test_overlap_constants():
    """The committed MACs are what their searches find, and meet their conditions."""
    for kind, consts in W.OVERLAP.items():
        assert consts, kind
        for free in sorted({f for f, _ in consts}):
            found = W.search_overlap(kind, [free], want=1 << 20)
            assert set(found) >= {(f, m) for f, m in consts if f == free}, (kind, free, found)
        for free, mac in consts:
            p, ci, ch = W.overlap_path(kind, free, mac)
            p += W.P.PAYLOAD
            w = W.walk(p, len(p), 1)
            assert w.status == "SCION_FORWARD" and w.clob == (True, False) and w.d == (8 if kind.startswith("d8") else 0)
            assert W.mac_ok(p, w) == (not kind.endswith("_after")), (kind, mac)
            assert W.mac_ok(p, w, after=True, rule=4) == kind.endswith("_after"), (kind, mac)
    assert W.OVERLAP["d8"][0][1] == "a2632378128d" and W.OVERLAP["d0"][0] == (63, "57f99d6fc0c4")
    # d0: forwarded with ConsIngress rewritten to 0002 ^ 57f9
    p, _, _ = W.overlap_path("d0", 63, "57f99d6fc0c4")
    w = W.walk(p + W.P.PAYLOAD, len(p) + 12, 1)
    assert w.stores == [(12 + 2, 0x57FB)] and w.meta_out >> 24 == 0x41
    for mac in W.OVERLAP_D4_MACS:                            # d4: the store zeroes MAC[0:2]
        p, _, _ = W.overlap_path("d4", 0, mac)
        w = W.walk(p + W.P.PAYLOAD, len(p) + 12, 1)
        assert w.d == 4 and w.stores == [(24 + 6, 0)] and not W.mac_ok(p, w) and not W.mac_ok(p, w, after=True, rule=4)


# ---- the corpus ---------------------------------------------------------------------------------

@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_placement_table(v6):
    """The counts of br_walk.ROWS, every one non-empty, and the table's shape."""
    recs = W.placement(v6)
    assert len(recs) == W.N_FRAMES == W.corpus(v6).n
    names = collections.Counter(n for _, ns in recs for n in ns)
    assert dict(names) == W.ROWS
    assert all(v > 0 for v in W.ROWS.values())
    table = collections.Counter(k for k, _ in recs)
    fwd = [k for k in table if k[0] == V["SCION_FORWARD"]]
    assert {k[1] for k in fwd if k[4]} == {0, 1, 2, 3} and {k[2] for k in fwd if k[4] and k[1] == 3} == {0}
    assert {k[3] for k in fwd} == {1, 2, -63, -62, 0}        # 0: a frame between siblings, not advanced
    assert {k[8] for k in fwd} == set(W.DIRECTIONS)
    # the five overlap rows: (verdict, d, MAC valid before, after)
    got = {(k[0], k[5], k[6], k[7]) for k in table if k[5] is not None and k[8] == "ext" and k[6] is not None}
    assert {(12, 8, True, False), (81, 8, False, True), (12, 0, True, False), (81, 0, False, True),
            (81, 4, False, False)} <= got
    assert (12, 8, True, True) not in got and not any(k[0] == 12 and k[6] is False for k in table)


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_case_a_frames_and_twins(v6):
    c = W.corpus(v6)
    (_, verdict, _, _), out = W.expected(v6)
    a = (c.kind == "base") & (c.what == "A")
    assert a.sum() == 2364 and (verdict[a] == V["SCION_FORWARD"]).all()
    flip, dc = c.kind == "flip", c.kind == "dontcare"
    assert flip.sum() == 2 * a.sum() and (verdict[flip] == V["INVALID_HF"]).all()
    assert dc.sum() == a.sum() and (verdict[dc] == V["SCION_FORWARD"]).all()
    assert set(c.what[dc]) == {"hf0", "inf1"}
    per = collections.Counter(zip(c.what[flip].tolist(), c.direction[flip].tolist()))
    for what in W.FLIPS:                                     # every field is flipped from every side with a MAC check
        for d in ("ext", "sib", "int"):
            assert per[(what, d)] >= 20, (what, d, per[(what, d)])
    for i in np.nonzero(flip | dc)[0]:                       # a twin differs from its frame in one bit of the path
        base = c.items[c.items[i].base]
        x = np.frombuffer(c.items[i].path, np.uint8) ^ np.frombuffer(base.path, np.uint8)
        assert np.unpackbits(x).sum() == 1
    assert not ((c.direction == "ipfwd") & a).any()          # no MAC check between siblings
    short = c.kind == "short"
    assert short.sum() == 108 and (verdict[short] == V["NOT_IMPLEMENTED"]).all()
    assert (c.lens[short] == [c.P + len(c.items[i].path) for i in np.nonzero(short)[0]]).all()


@pytest.mark.parametrize("hf_check", [True, False], ids=["hf_check", "hf_check_off"])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_checker_against_the_model(v6, hf_check):
    """Verdict, egress and every path byte of every frame, by the model's integers."""
    c = W.corpus(v6)
    (_, verdict, egress, _), out = W.expected(v6, hf_check)
    for i in range(c.n):
        mv, me, mo, w = c.judge(i, hf_check)
        plen = max(int(c.lens[i]) - c.P, 0)
        got = out[i, c.P:c.P + plen].tobytes()
        assert (mv, me) == (verdict[i], egress[i]) and got == mo[:plen], (i, c.items[i].kind, c.items[i].what, w.status)
        assert (out[i, c.lens[i]:] == c.frames[i, c.lens[i]:]).all()
    if not hf_check:                                         # every overlap frame, the twins included, forwards
        assert (verdict[c.kind == "overlap"] == V["SCION_FORWARD"]).all()
        assert not (verdict == V["INVALID_HF"]).any()


@pytest.mark.parametrize("hf_check", [True, False], ids=["hf_check", "hf_check_off"])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_checker_against_the_reference_program(v6, hf_check):
    if not orc.ref_br_available(hf_check):
        pytest.skip("reference router not built (oracle/_ref)")
    c = W.corpus(v6)
    res, out = W.expected(v6, hf_check)
    prog = c.frames.copy()
    orc.assert_br_equal(res, out, orc.ref_br_process(prog, c.lens, c.ifidx, c.cfg, W.HK, hf_check=hf_check), prog,
                        "checker against the reference program")


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_checker_against_the_fixture(v6):
    """tests/golden/br_walk.npz: what the reference program gave for the corpus."""
    c = W.corpus(v6)
    res, out = W.expected(v6)
    g, fam = orc.load_golden("br_walk.npz"), "v6" if v6 else "v4"
    assert g["sha256_" + fam].tobytes() == S.sha256(c.frames, c.lens, c.ifidx), "the generator drifted"
    want = c.frames.copy()
    want[:, :W.FIXTURE_WIDTH] ^= g["xor_" + fam]
    orc.assert_br_equal(res, out, (g["action_" + fam], g["verdict_" + fam], g["egress_" + fam], g["stats_" + fam]), want,
                        "checker against the fixture")


def test_without_a_key_nothing_verifies():
    c = W.corpus(False)
    (_, verdict, _, _), _ = W.expected(False, key=False)
    (_, with_key, _, _), _ = W.expected(False)
    checked = np.isin(with_key, [V["SCION_FORWARD"], V["INVALID_HF"]]) & (c.direction != "ipfwd")
    hit = np.array([bool(c.walk(i).mac) and c.walk(i).status == "SCION_FORWARD" for i in range(c.n)])
    assert (verdict[hit] == V["INVALID_HF"]).all() and (verdict[~hit] == with_key[~hit]).all() and hit.sum() > 5000
    assert (hit <= checked).all()


# ---- the wrong rules ----------------------------------------------------------------------------

@pytest.mark.parametrize("rule", W.RULES)
def test_wrong_rule_changes_the_corpus(rule):
    """Each wrong step of `make pathwalk`, restated in the model, changes the verdict, the egress or an
    output byte of at least one frame: the corpus can tell it from the reference's rule."""
    c = W.corpus(False)
    hits = collections.Counter()
    for i in range(c.n):
        p, plen = c.path(i)
        if rule == 9:
            if W.locate(p, plen, 9) != W.locate(p, plen):
                hits[c.items[i].kind] += 1
            continue
        mv, me, mo, _ = c.judge(i)
        rv, re_, ro, _ = c.judge(i, rule=rule)
        if (mv, me) != (rv, re_) or mo[:max(plen, 0)] != ro[:max(plen, 0)]:
            hits[(c.items[i].kind, mv, rv)] += 1
    assert sum(hits.values()) >= {4: 5, 5: 5, 7: 100}.get(rule, 30), hits
    if rule in (4, 5):                                       # only the overlap class tells these two
        assert {k[0] for k in hits} == {"overlap"} or {k[0] for k in hits} <= {"overlap", "trunc"}, hits
        assert (("overlap", V["SCION_FORWARD"], V["INVALID_HF"]) in hits) and (("overlap", V["INVALID_HF"], V["SCION_FORWARD"]) in hits)
    if rule == 7:                                            # NOT_IMPLEMENTED at the path's end becomes PARSE_ERROR
        assert hits[("short", V["NOT_IMPLEMENTED"], V["PARSE_ERROR"])] == 108


# ---- the host parser ----------------------------------------------------------------------------

@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_host_parser_against_the_model(v6):
    """hfv_frame_locate: status and offsets; hfv_frame_extract: the 8 + 12 bytes, with MAC[0:2] folded
    into the SegID of a Cons = 0 info field for a frame from the internal link."""
    import ctypes
    c = W.corpus(v6)
    L = hfv.lib()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    base = c.frames.ctypes.data
    want_inf = np.zeros((c.n, 8), np.uint8)
    want_hf = np.zeros((c.n, 12), np.uint8)
    want_st = np.zeros(c.n, np.uint8)
    deep = 0
    for i in range(c.n):
        p, plen = c.path(i)
        st, inf, hf = W.locate(p, plen)
        rc = L.hfv_frame_locate(base + i * W.SLOT, int(c.lens[i]), ctypes.byref(a), ctypes.byref(b))
        assert rc == st, (i, rc, st)
        want_st[i] = st
        if st == 0:
            assert (a.value, b.value) == (c.P + inf, c.P + hf), i
            want_inf[i], want_hf[i] = np.frombuffer(p[inf:inf + 8], np.uint8), np.frombuffer(p[hf:hf + 12], np.uint8)
            if c.internal[i] and not p[inf] & 1:
                want_inf[i, 2:4] ^= want_hf[i, 6:8]
            deep += hf > 700
    assert deep > 100 and (want_st == 0).sum() > 14000 and (want_st == hfv.FRAME_PARSE_ERROR).sum() > 2000
    st, inf, hf = R.frame_extract(c.frames, c.lens, c.internal)
    assert np.array_equal(st, want_st)
    ok = st == 0
    assert np.array_equal(inf[ok], want_inf[ok]) and np.array_equal(hf[ok], want_hf[ok])
    assert not inf[~ok].any() and not hf[~ok].any()
