"""The oracle border router (oracle/hfv_br_oracle.c) against the reference's own router program:
br/src/bpf/xdp.c compiled as host code (oracle/_ref/librefbr*.so, driver oracle/ref_br.c), bit
for bit on frames (every byte of every slot), XDP action, verdict, redirect target and counters.

Where the reference build is absent the comparison tests skip and the committed fixture
tests/golden/br_ref.npz (the reference build's outputs, tests/golden/make_golden.py) still pins
the oracle.  The GPU router is compared with the same judge in tests/test_gpu_br.py.
"""
import os
import sys

import numpy as np
import pytest

import br_fuzz as F
import br_topo as T
import orc
import scion_hfv as hfv

V = hfv.VERDICT
MAC = lambda k, m: orc.cmac(m, k)   # noqa: E731
needs_ref = pytest.mark.skipif(not orc.ref_br_available(), reason="reference router not built (oracle/_ref)")


def check(frames, lens, ifidx, cfg, key0=T.KEYS[1], hf_check=True, feat_off=0, what=""):
    """Oracle and reference program over copies of the batch; returns the reference's results."""
    hk = orc.hop_key(key0) if key0 is not None else None
    a = frames.copy()
    o = orc.br_process(a, lens, ifidx, cfg, hk, hf_check=hf_check, feat_off=feat_off)
    b = frames.copy()
    assert feat_off in (0, hfv.BR_NO_IPV6)
    r = orc.ref_br_process(b, lens, ifidx, cfg, hk, hf_check=hf_check, no_ipv6=feat_off == hfv.BR_NO_IPV6)
    assert r is not None, "this variant of the reference router is not built"
    orc.assert_br_equal(o, a, r, b, what)
    return r, b


@pytest.fixture(scope="module")
def hops():
    out = {}
    for v6 in (False, True):
        brs = {b: T.OracleBR(T.br_config(b, v6)) for b in ("br1", "br2", "br3")}
        out[v6] = F.hop_inputs(brs, v6, MAC)
    return out


# ---- every batch of tests/test_br_oracle.py -------------------------------------------------------
@needs_ref
def test_oracle_suite_under_the_reference(monkeypatch):
    """tests/test_br_oracle.py once more, with every oracle call it makes (the PTF chains, the
    hand-made frames of every process_packet exit, its fuzz batches) also run through the
    reference program and compared.  Calls with a build option the reference cannot be compiled
    with (ENABLE_IPV4 or ENABLE_SCION_PATH off) are counted, not compared."""
    import test_br_oracle as O
    real = orc.br_process
    seen = {"compared": 0, "unpinned": 0}

    def checked(frames, lens, ifidx, cfg, key0_hop_key=None, stats=None, hf_check=True, feat_off=0):
        before = frames.copy()
        s0 = None if stats is None else stats.copy()
        res = real(frames, lens, ifidx, cfg, key0_hop_key, stats, hf_check, feat_off)
        if feat_off not in (0, hfv.BR_NO_IPV6) or (feat_off and not hf_check):
            seen["unpinned"] += 1
            return res
        r = orc.ref_br_process(before, lens, ifidx, cfg, key0_hop_key, hf_check=hf_check,
                               no_ipv6=feat_off == hfv.BR_NO_IPV6, stats=s0)
        orc.assert_br_equal(res, frames, r, before, "oracle call %d" % seen["compared"])
        seen["compared"] += 1
        return res

    monkeypatch.setattr(orc, "br_process", checked)
    for v6 in (False, True):
        topo = (v6, {b: T.OracleBR(T.br_config(b, v6)) for b in ("br1", "br2", "br3")})
        O.test_ptf_scenarios(topo)
        O.test_fuzz_is_deterministic_and_covers_verdicts(topo)
        O.test_segid_rewrite_inside_checked_hop_field(v6)
    for t in (O.test_not_scion_and_parse_errors, O.test_interface_checks, O.test_router_alert_and_last_hop,
              O.test_bad_mac_and_missing_key, O.test_hf_check_off_forwards_bad_macs, O.test_build_options,
              O.test_unknown_egress_aborts_and_falls_through, O.test_fib_outcomes, O.test_underlay_mismatch,
              O.test_ipv4_options_move_fields_not_outcomes):
        t()
    assert seen["compared"] >= 100 and seen["unpinned"] == 4, seen


# ---- every batch of tests/test_gpu_br.py ---------------------------------------------------------
def _mixed_family_batch(hops):
    mix = [F.fuzz_batch(hops[v6], "br1", v6, 4000, seed=300 + v6) for v6 in (False, True)]
    frames = np.concatenate([mix[0][0], mix[1][0]])
    lens = np.concatenate([mix[0][1], mix[1][1]])
    ifidx = np.concatenate([mix[0][2], mix[1][2]])
    order = np.random.default_rng(5).permutation(len(frames))
    return np.ascontiguousarray(frames[order]), lens[order], ifidx[order]


@needs_ref
@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_gpu_suite_batches_per_family(hops, v6):
    """The batches of test_gpu_br.py that exist per family, generators and seeds as there."""
    for br in ("br1", "br2", "br3"):
        frames, lens, ifidx = F.fuzz_batch(hops[v6], br, v6, 20000, seed=100 + v6, payload_max=1500)
        r, _ = check(frames, lens, ifidx, T.br_config(br, v6), what="fuzz_parity " + br)
        assert len(np.unique(r[1])) >= 6
    frames, lens, ifidx = F.fuzz_batch(hops[v6], "br1", v6, 20000, seed=200 + v6, payload_max=1500)
    for key0 in (T.KEYS[1], None):
        r, _ = check(frames, lens, ifidx, T.br_config("br1", v6), key0, hf_check=False, what="hf_check off")
        assert V["INVALID_HF"] not in r[1]
    frame, first, ifi, want = F.overlap_frame(v6)
    rest = [(f, i) for b, i, f in hops[v6] if b == first][:63]
    frames, lens = T.to_slots([frame] + [f for f, _ in rest])
    ifidx = np.array([ifi] + [i for _, i in rest], dtype=np.uint32)
    r, out = check(frames, lens, ifidx, T.br_config(first, v6), what="overlap tile")
    assert r[1][0] == V["SCION_FORWARD"] and out[0, :len(want)].tobytes() == want


@needs_ref
def test_gpu_suite_batches_ipv4(hops):
    h = hops[False]
    cfg = T.br_config("br1")
    frames, lens, ifidx, m = F.options_shift_batch(h)
    check(frames, lens, ifidx, cfg, what="options shift")
    for hdrlen in (0, 23, 255):
        f2 = frames.copy()
        for i in range(len(f2)):
            f2[i, 14 + 4 * (f2[i, 14] & 15) + 8 + 5] = hdrlen
        check(f2, lens, ifidx, cfg, what="hdrlen %d" % hdrlen)
    frames, lens, ifidx = F.fuzz_batch(h, "br1", False, 4000, seed=7)
    for key0 in (None, T.KEYS[5]):
        check(frames, lens, ifidx, cfg, key0, what="no key / foreign key")
    frames, lens, ifidx = F.fuzz_batch(h, "br1", False, (1 << 14) + 37, seed=11, payload_max=1500)
    check(frames, lens, ifidx, cfg, what="split launch batch")
    for n, seed, slot in ((3000, 5, 512), (2000, 17, 512)):
        frames, lens, ifidx = F.fuzz_batch(h, "br1", False, n, seed=seed, slot=slot)
        check(frames, lens, ifidx, cfg, what="host path slot 512")
    frames, lens, ifidx = F.fuzz_batch(h, "br1", False, 3000, seed=31)
    for name in ("br1", "br2"):
        check(frames, lens, ifidx, T.br_config(name), what="pinned brconfig " + name)
    # test_stats_accumulate_and_bad_args: one frame 100 times, then its own output once more
    from scion_hfv import packets as P
    ing_enc, _, _, ifi = T.encaps(1, 2, False)
    frame = ing_enc.frame(P.scion_header(P.ptf_path("down", 1, 2, T.KEYS, seed=9, mac_fn=MAC).pack()))
    buf, lens = T.to_slots([frame] * 100)
    ifidx = np.full(100, ifi, dtype=np.uint32)
    r, out = check(buf, lens, ifidx, cfg, what="stats pass 1")
    r2, _ = check(out, lens, ifidx, cfg, what="stats pass 2")
    assert (r[1] == V["SCION_FORWARD"]).all() and (r2[1] == V["NO_INTERFACE"]).all()


@needs_ref
def test_gpu_suite_batch_unstaged_slot(hops):
    frames, lens, ifidx = F.fuzz_batch(hops[True], "br1", True, 6000, seed=9, slot=1032, payload_max=1000)
    check(frames, lens, ifidx, T.br_config("br1", True), what="slot 1032")


@needs_ref
def test_gpu_suite_host_path_batch(hops):
    frames, lens, ifidx = F.fuzz_batch(hops[False], "br1", False, 70000, seed=21, payload_max=1500)
    longf = F.long_path_frames(False, MAC)
    for k, (f, ifi) in enumerate(longf):
        i = 1000 + k * 8191
        frames[i] = 0
        frames[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        lens[i], ifidx[i] = len(f), ifi
    r, _ = check(frames, lens, ifidx, T.br_config("br1"), what="host path batch")
    assert (r[0][[1000 + k * 8191 for k in range(len(longf))]] == 4).all()


@needs_ref
def test_gpu_suite_large_batch(hops):
    """The 2^17-frame batch of test_large_batch_mixed_sizes."""
    frames, lens, ifidx = F.fuzz_batch(hops[False], "br1", False, 1 << 17, seed=3, payload_max=1500)
    check(frames, lens, ifidx, T.br_config("br1"), what="2^17 batch")


@needs_ref
@pytest.mark.parametrize("hf_check", [True, False], ids=["hf_check", "hf_check_off"])
def test_gpu_suite_bench_batch(hf_check):
    """The 2^20-frame batch the config-4 bench times (test_bench_batch_full_size_bit_exact), in
    pieces of 2^16 frames so that only 128 MiB of slots exist at a time."""
    sys.path.insert(0, orc.ROOT)
    import bench
    n = 1 << 20
    tmpl, tid, lens, ifidx, n_good = bench.br_batch(n, 0)
    cfg = T.br_config("br1")
    fwd = 0
    for lo in range(0, n, 1 << 16):
        sl = slice(lo, lo + (1 << 16))
        r, _ = check(tmpl[tid[sl]], lens[sl], ifidx[sl], cfg, hf_check=hf_check, what="bench batch at %d" % lo)
        fwd += int((r[0] == 4).sum())
    assert fwd == (n_good if hf_check else n)


@needs_ref
@pytest.mark.skipif(not orc.ref_br_available(no_ipv6=True), reason="ENABLE_IPV6=OFF reference build absent")
def test_build_without_ipv6(hops):
    """feat_off = ORC_BR_NO_IPV6 against the reference compiled without ENABLE_IPV6, on the mixed
    batch of test_fuzz_parity_build_options.  (The reference does not compile without
    ENABLE_IPV4 or ENABLE_SCION_PATH, so the two other options have no reference build.)"""
    frames, lens, ifidx = _mixed_family_batch(hops)
    r, _ = check(frames, lens, ifidx, T.br_config("br1", False), feat_off=hfv.BR_NO_IPV6, what="no_ipv6")
    assert V["SCION_FORWARD"] in r[1] and V["NOT_SCION"] in r[1]
    check(frames, lens, ifidx, T.br_config("br1", False), what="same batch, all families")


# ---- hostile input -----------------------------------------------------------------------------
def hostile_batch(hops_v, v6, n, seed):
    """A fuzz batch with 1-3 random byte changes in bytes 12-159 of every frame, 20 % of the
    frames cut at a random length and 10 % arriving on a random ifindex in 0..69."""
    frames, lens, ifidx = F.fuzz_batch(hops_v, "br1", v6, n, seed, slot=256)
    rng = np.random.default_rng([seed, 1])
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            frames[i, int(rng.integers(12, 160))] = int(rng.integers(0, 256))
    cut = rng.random(n) < 0.2
    lens[cut] = rng.integers(0, 257, int(cut.sum()))
    port = rng.random(n) < 0.1
    ifidx[port] = rng.integers(0, 70, int(port.sum()))
    return frames, lens, ifidx


@needs_ref
@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_hostile_frames(hops, v6):
    frames, lens, ifidx = hostile_batch(hops[v6], v6, 30000, seed=41 + v6)
    r, _ = check(frames, lens, ifidx, T.br_config("br1", v6), what="hostile")
    assert len(np.unique(r[1])) >= 8


@needs_ref
def test_random_bytes():
    """20000 slots of pure random bytes with random lengths (0..slot and beyond) and ports; a
    tenth get an EtherType and protocol that lets them past parse_underlay."""
    rng = np.random.default_rng(77)
    n, slot = 20000, 256
    frames = rng.integers(0, 256, (n, slot), dtype=np.uint8)
    lens = rng.integers(0, slot + 40, n).astype(np.uint16)
    ifidx = rng.choice(F.IFINDICES, n).astype(np.uint32)
    k = n // 10
    frames[:k, 12:14] = (0x08, 0x00)
    frames[:k, 23] = 17
    frames[k:2 * k, 12:14] = (0x86, 0xDD)
    frames[k:2 * k, 20] = 17
    for v6 in (False, True):
        r, _ = check(frames, lens, ifidx, T.br_config("br1", v6), what="random bytes")
        assert V["PARSE_ERROR"] in r[1] and V["NOT_SCION"] in r[1]


@needs_ref
@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_ptf_long_paths_and_hop_inputs(hops, v6):
    """Every frame of the PTF scenarios as it enters each router of the chain, and the long
    3-segment paths, each under the table of the router that sees it."""
    for br in ("br1", "br2", "br3"):
        mine = [(i, f) for b, i, f in hops[v6] if b == br]
        frames, lens = T.to_slots([f for _, f in mine])
        r, _ = check(frames, lens, np.array([i for i, _ in mine], dtype=np.uint32), T.br_config(br, v6), what=br)
        assert (r[1] == V["SCION_FORWARD"]).all()
    longf = F.long_path_frames(v6, MAC)
    frames, lens = T.to_slots([f for f, _ in longf])
    r, _ = check(frames, lens, np.array([i for _, i in longf], dtype=np.uint32), T.br_config("br1", v6), what="long")
    assert (r[0] == 4).all()


# ---- table fuzz ----------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_table_fuzz(hops, v6):
    """Every mutated table of br_fuzz.config_cases on the 1024-frame batch; and the conditions
    the case list has to meet, counted on the reference's own verdicts: each of the 11 verdict
    values in at least 8 frames, UNDERLAY_MISMATCH and FIB_LKUP_DROP each under 3 tables."""
    frames, lens, ifidx = F.table_fuzz_batch(hops[v6], v6)
    f2, l2, i2 = F.table_fuzz_batch(hops[v6], v6)
    assert (frames == f2).all() and (lens == l2).all() and (ifidx == i2).all()
    cases = F.config_cases(v6)
    again = F.config_cases(v6)
    assert len(cases) == F.TABLE_FUZZ_COUNT and [bytes(c) for c in cases] == [bytes(c) for c in again]
    count = np.zeros(256, dtype=np.int64)
    tables = np.zeros(256, dtype=np.int64)
    for n, c in enumerate(cases):
        assert 1 <= len(c.mutations) <= 3
        assert all(0 <= c.routes[i].ret <= 8 for i in range(c.n_routes))
        r, _ = check(frames, lens, ifidx, c, what="table case %d %s" % (n, c.mutations))
        hist = np.bincount(r[1], minlength=256)
        count += hist
        tables += hist > 0
    values = sorted(V.values())
    assert len(values) == 11
    assert all(count[v] >= 8 for v in values), {v: int(count[v]) for v in values}
    assert count.sum() == sum(count[v] for v in values)
    assert tables[V["UNDERLAY_MISMATCH"]] >= 3 and tables[V["FIB_LKUP_DROP"]] >= 3


@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_route_result_outside_0_8_is_success(hops, v6):
    """hfv_br_config.h: a route result other than 0..8 is treated as success.  The reference
    program defines nothing there, so the oracle is judged against itself with that result set
    to 0 -- frames, verdicts, egress and counters must not change."""
    frames, lens, ifidx = F.table_fuzz_batch(hops[v6], v6)
    hk = orc.hop_key(T.KEYS[1])
    cases = F.config_cases_undefined_ret(v6)
    assert {c.routes[i].ret for c in cases for i in range(c.n_routes)} >= set(F.UNDEFINED_RETS)
    for c in cases:
        z = F._clone(c)
        for i in range(z.n_routes):
            if not 0 <= z.routes[i].ret <= 8:
                z.routes[i].ret = 0
        a, b = frames.copy(), frames.copy()
        orc.assert_br_equal(orc.br_process(a, lens, ifidx, c, hk), a, orc.br_process(b, lens, ifidx, z, hk), b,
                            str(c.mutations))


# ---- the committed fixture -----------------------------------------------------------------------
def _fixture_runs(process):
    g = orc.load_golden("br_ref.npz")
    hk = orc.hop_key(g["key0"].tobytes())
    assert g["frames"].shape == (2, F.TABLE_FUZZ_N, F.TABLE_FUZZ_SLOT) and g["cfgs"].shape[1] == 8
    seen = set()
    for fam in range(2):
        for t in range(g["cfgs"].shape[1]):
            cfg = hfv.BrConfig.from_buffer_copy(g["cfgs"][fam, t].tobytes())
            got = g["frames"][fam].copy()
            res = process(got, g["lens"][fam], g["ifidx"][fam], cfg, hk)
            want = (g["action"][fam, t], g["verdict"][fam, t], g["egress"][fam, t], g["stats"][fam, t])
            orc.assert_br_equal(res, got, want, g["frames"][fam] ^ g["frames_out_xor"][fam, t],
                                "fixture family %d table %d" % (fam, t))
            seen |= set(np.unique(g["verdict"][fam, t]).tolist())
        assert seen == set(V.values())


def test_oracle_reproduces_reference_fixture():
    _fixture_runs(orc.br_process)


@needs_ref
def test_reference_reproduces_its_fixture(hops):
    """The check make_golden.py makes: the fixture is what the reference build computes now, from
    inputs that are still what the generators give."""
    _fixture_runs(orc.ref_br_process)
    g = orc.load_golden("br_ref.npz")
    for fam, v6 in enumerate((False, True)):
        frames, lens, ifidx = F.table_fuzz_batch(hops[v6], v6)
        assert (g["frames"][fam] == frames).all() and (g["lens"][fam] == lens).all() and (g["ifidx"][fam] == ifidx).all()
        mine = {bytes(c) for c in F.config_cases(v6)}
        assert all(g["cfgs"][fam, t].tobytes() in mine for t in range(8))


@needs_ref
def test_scratchpad_carry_over_switch(hops):
    """refbr's carry switch keeps the per-CPU scratchpad across frames, as XDP does; the oracle's
    (and the kernel's) per-frame zeroing is the one documented deviation.  DESIGN.md section 2
    records how many frames of the fixture batch change; here only that the switch works and
    that no verdict, action or redirect target depends on it."""
    g = orc.load_golden("br_ref.npz")
    hk = orc.hop_key(g["key0"].tobytes())
    for fam in range(2):
        cfg = T.br_config("br1", bool(fam))
        a, b = g["frames"][fam].copy(), g["frames"][fam].copy()
        z = orc.ref_br_process(a, g["lens"][fam], g["ifidx"][fam], cfg, hk)
        c = orc.ref_br_process(b, g["lens"][fam], g["ifidx"][fam], cfg, hk, carry=True)
        assert (z[0] == c[0]).all() and (z[1] == c[1]).all() and (z[2] == c[2]).all() and (z[3] == c[3]).all()
        again = g["frames"][fam].copy()
        orc.ref_br_process(again, g["lens"][fam], g["ifidx"][fam], cfg, hk)
        assert (again == a).all()        # the switch was reset: zeroed scratchpad again
