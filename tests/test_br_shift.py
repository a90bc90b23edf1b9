"""The window-edge corpus of tests/br_shift.py on the CPU: the shifted frames are routed as their
bases are (oracle router, and the reference's own program where it is built), the corpus puts
every header field in front of, across and past bytes 128 and 136 (asserted cell by cell), the
host parser agrees with the placement rule, and tests/golden/br_shift.npz records what the
reference program gave.  Integer work: every comparison is exact."""
import numpy as np
import pytest

import br_shift as S
import br_topo as T
import orc
import scion_hfv as hfv

V = hfv.VERDICT
HK = orc.hop_key(T.KEYS[1])
FAMILIES = pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
needs_ref = pytest.mark.skipif(not orc.ref_br_available(), reason="reference router not built (oracle/_ref)")


def corpus_oracle(br, v6):
    return S.oracle(S.corpus_name(br, v6))


def sweep_oracle(v6):
    return S.oracle(S.sweep_name(v6))


def all_corpora(brs=S.BRS):
    return [S.shift_corpus(v6)[br] for v6 in (False, True) for br in brs]


# ---- invariance ---------------------------------------------------------------------------------

@FAMILIES
def test_shifted_frames_are_routed_as_their_bases(v6):
    shifts = S.V6_SHIFTS if v6 else S.V4_SHIFTS
    counts = {"br1": 36, "br2": 24, "br3": 12}
    for br in S.BRS:
        fr, ln, ifi, sid, bid = S.shift_corpus(v6)[br]
        m = counts[br]
        assert len(fr) == m * len(shifts) and ln.max() <= (206 if v6 else 226)
        (a, v, e, _), out = corpus_oracle(br, v6)
        assert (a == 4).all() and (v == V["SCION_FORWARD"]).all()           # every corpus frame is forwarded
        assert shifts[0] == (0, 0) and (sid[:m] == 0).all() and (bid[:m] == np.arange(m)).all()
        assert (e == e[bid]).all() and (ifi == ifi[bid]).all()
        for i in range(len(fr)):
            k, j = shifts[sid[i]]
            b = int(bid[i])
            assert S.unshifted(bytes(fr[i, :ln[i]]), v6, k, j) == bytes(fr[b, :ln[b]])   # the rule inverts
            got = bytearray(S.unshifted(bytes(out[i, :ln[i]]), v6, k, j))
            want = bytearray(out[b, :ln[b]])
            if not v6:       # the shifted frame's IPv4 header checksum is stale and updated incrementally
                got[24:26] = want[24:26] = b"\0\0"
            assert got == want, (br, i, k, j)
            assert not out[i, ln[i]:].any()
        assert (out != fr).any(axis=1).all()


# ---- coverage, as asserted conditions -----------------------------------------------------------

# field -> edge -> (in, {bytes in front of the edge: frames}, past), over the 2592 frames
PLACEMENT = {
    "meta": {128: (2304, {2: 144}, 144), 136: (2520, {2: 72}, 0)},
    "seg0": {128: (2097, {}, 495), 136: (2412, {}, 180)},
    "seg1": {128: (207, {}, 117), 136: (270, {}, 54)},
    "hf": {128: (342, {2: 198, 6: 243, 10: 180}, 1629), 136: (765, {2: 207, 6: 270, 10: 198}, 1152)},
    "mac": {128: (342, {4: 180}, 2070), 136: (765, {4: 198}, 1629)},
}


def test_placement_table():
    corpora = all_corpora()
    assert sum(len(c[0]) for c in corpora) == 2592
    assert [sum(len(S.shift_corpus(v6)[br][0]) for br in S.BRS) for v6 in (False, True)] == [2376, 216]
    metas = sorted({S.field_offsets(f)["meta"][0] for f in S.corpus_frames(corpora)})
    assert metas == list(range(78, 135, 4))
    table = S.placement_table(corpora, S.EDGES)
    for field, per_edge in PLACEMENT.items():
        for edge, (n_in, straddle, past) in per_edge.items():
            assert table[(field, edge)] == {"in": n_in, "straddle": straddle, "past": past}, (field, edge)
    assert sum(PLACEMENT["hf"][128][1].values()) == 621 and sum(PLACEMENT["hf"][136][1].values()) == 675
    assert PLACEMENT["seg1"][128][0] + PLACEMENT["seg1"][128][2] == 324      # frames with a segment switch


def test_placement_table_br1_alone():
    """Several GPU legs run br1 only: every non-zero cell of the table is non-zero there too."""
    table = S.placement_table(all_corpora(("br1",)), S.EDGES)
    for field, per_edge in PLACEMENT.items():
        for edge, (n_in, straddle, past) in per_edge.items():
            cell = table[(field, edge)]
            assert (cell["in"] > 0) == (n_in > 0) and (cell["past"] > 0) == (past > 0), (field, edge)
            assert set(cell["straddle"]) == set(straddle), (field, edge)


def test_host_path_windows_split_the_corpus():
    """A header window of W bytes holds a frame's headers or does not (then the host path re-runs
    the frame whole).  The shortest headers of the corpus end at byte 114 (IPv4: PathMeta at 78, one
    info field, the second hop field) and 134 (IPv6), so both kinds exist for every W the GPU test
    uses from 120 (IPv6: 136) to 160, in br1 alone, and no frame fits W = 64, 88, 104 or 112."""
    for v6, lowest, highest in ((False, 114, 190), (True, 134, 170)):
        for br in S.BRS:
            ends = np.array([S.header_end(f) for f in S.corpus_frames(S.shift_corpus(v6)[br])])
            assert (ends.min(), ends.max()) == (lowest, highest)
            for w in S.HOST_WINDOWS + S.HOST_WINDOWS_ALL_ABOVE:
                both = (ends <= w).any() and (ends > w).any()
                assert both == (lowest <= w), (v6, br, w)
                assert both or (ends > w).all()
    assert [w for w in S.HOST_WINDOWS if w >= 114] == [120, 128, 136, 144, 152, 160]


# ---- judges -------------------------------------------------------------------------------------

@needs_ref
@FAMILIES
def test_oracle_against_the_reference_program(v6):
    for name, br, fam, fr, ln, ifi in S.fixture_legs():
        if fam != v6:
            continue
        res, out = S.oracle(name)
        prog = fr.copy()
        ref = orc.ref_br_process(prog, ln, ifi, T.br_config(br, v6), HK)
        orc.assert_br_equal(res, out, ref, prog, name)


@FAMILIES
def test_truncation_sweep_verdicts(v6):
    fr, ln, ifi = S.truncation_sweep(v6)
    assert 2500 <= len(fr) <= 5000 and len(fr) == sum(
        len(f) + (8 * j + 4 * k) + 1 for _, _, f, _ in S.sweep_bases(v6)
        for j, k in ([(j, 0) for j in S.SWEEP_V6] if v6 else S.SWEEP_V4))
    (a, v, e, _), out = sweep_oracle(v6)
    for name in ("PARSE_ERROR", "NOT_SCION", "SCION_FORWARD"):
        assert (v == V[name]).sum() >= 15, name
    full = np.nonzero(np.diff(ln.astype(np.int64), append=0) <= 0)[0]       # the untruncated frame of each run
    assert len(full) == 5 * (3 if v6 else 5) and (v[full] == V["SCION_FORWARD"]).all()
    assert (out[a != 4] == fr[a != 4]).all()                                # only forwarded frames are rewritten


def locate(row, ln):
    return hfv.lib().hfv_frame_locate(bytes(row), int(ln), *_U32)


_U32 = (hfv.ctypes.byref(hfv.ctypes.c_uint32()), hfv.ctypes.byref(hfv.ctypes.c_uint32()))


def test_host_parser_against_the_placement_rule():
    """hfv_frame_locate / hfv_frame_extract (the parser the extract kernels share) on the corpus:
    status 0, and the current info and hop field where field_offsets puts them."""
    for c in all_corpora():
        for f in S.corpus_frames(c):
            o = S.field_offsets(f)
            assert hfv.frame_locate(f) == (0, o["inf_off"], o["hf_off"])
            st, inf, hf = hfv.frame_extract(f)
            assert (st, inf, hf) == (0, f[o["inf_off"]:o["inf_off"] + 8], f[o["hf_off"]:o["hf_off"] + 12])


@FAMILIES
def test_host_parser_status_on_the_truncation_sweep(v6):
    """A non-zero status is the verdict the router oracle records, and every frame the router
    calls NOT_SCION or NOT_IMPLEMENTED has that status (the mapping of test_frames_host.py)."""
    fr, ln, _ = S.truncation_sweep(v6)
    (_, v, _, _), _ = sweep_oracle(v6)
    st = np.array([locate(fr[i], ln[i]) for i in range(len(fr))])
    bad = st != 0
    assert np.array_equal(v[bad], st[bad])
    for name in ("NOT_SCION", "NOT_IMPLEMENTED"):
        assert (st[v == V[name]] == V[name]).all()
    assert bad.sum() >= 2000 and (~bad).sum() >= 300


# ---- the fixture --------------------------------------------------------------------------------

def check_fixture(g, name, res, out, frames, lens, ifidx):
    assert g[name + "_sha256"].tobytes() == S.sha256(frames, lens, ifidx), "the generator drifted: " + name
    want = (g[name + "_action"], g[name + "_verdict"], g[name + "_egress"], g[name + "_stats"])
    xor = g[name + "_xor"] if name + "_xor" in g else None
    if xor is None:             # no XOR plane recorded: outputs and counters only
        a, v, e, s = res
        assert np.array_equal(a, want[0]) and np.array_equal(v, want[1]) and np.array_equal(e, want[2]), name
        assert np.array_equal(np.asarray(s).reshape(orc.BR_STATS_SHAPE), want[3]), name
    else:
        orc.assert_br_equal(res, out, want, frames ^ xor, name)


def test_oracle_reproduces_the_fixture():
    """tests/golden/br_shift.npz: what the reference program gave for the corpus and the sweep
    (make_golden.py br_shift).  Needs no reference build."""
    g = orc.load_golden("br_shift.npz")
    for name, br, v6, fr, ln, ifi in S.fixture_legs():
        res, out = S.oracle(name)
        check_fixture(g, name, res, out, fr, ln, ifi)


@needs_ref
def test_reference_program_reproduces_the_fixture():
    g = orc.load_golden("br_shift.npz")
    for name, br, v6, fr, ln, ifi in S.fixture_legs():
        prog = fr.copy()
        res = orc.ref_br_process(prog, ln, ifi, T.br_config(br, v6), HK)
        check_fixture(g, name, res, prog, fr, ln, ifi)
