"""Parity of the resident verify service (hfv_service_*: persistent grid fed through the host
descriptor ring) against the CPU checker, the committed fixtures and the launch-per-batch
path.  Integer work: every comparison is bit-exact.

hfv_service_submit is host-ordered, not stream-ordered: a batch's records and bitmap must be
complete when it is posted, so the tests synchronize torch's stream after preparing them."""
import time

import numpy as np
import pytest

import key_tables as KT
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def new_bits(n, fill=0):
    return torch.full((max(1, (n + 63) // 64),), fill, dtype=torch.int64, device=DEV)


def bits_np(t, n):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)[: (n + 63) // 64]


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.service_stop()
    c.close()


@pytest.mark.parametrize("name,keysel", [("hf_single.npz", 0), ("hf_ifid256.npz", 1)])
def test_service_golden(ctx, name, keysel):
    g = orc.load_golden(name)
    n = len(g["records"])
    raw = g["raw_keys"].reshape(-1).tobytes()
    for k in range(int(g["nkeys"])):
        ctx.key_add(k, raw[16 * k:16 * k + 16])
    ctx.set_keysel(keysel)
    bits = new_bits(n, fill=-1)
    d = dev(g["records"])
    torch.cuda.synchronize()
    t = ctx.service_submit(d, n, bits)
    ctx.service_wait(t, 20000)
    assert ctx.service_poll(t)
    assert np.array_equal(bits_np(bits, n), g["pass_bits"])
    ms = ctx.service_stop()
    assert ms > 0 and not ctx.service_running


@pytest.mark.parametrize("keysel", [0, 1])
def test_service_ragged_batches_vs_oracle(ctx, keysel):
    """Many batches of ragged sizes (incl. 0, 1 and sizes smaller than the grid, where most
    blocks own no tile) in flight at once, each against the oracle."""
    rng = np.random.default_rng(21 + keysel)
    raw = orc.gen_key_table(256)
    hk, valid = orc.key_table(raw)
    for k in range(256):
        ctx.key_add(k, raw[16 * k:16 * k + 16])
    ctx.set_keysel(keysel)
    recs = orc.gen_records(41000, hk, keysel, seed=77)   # offsets < 1000 + sizes <= 40000
    junk = rng.random(len(recs)) < 0.2
    recs[junk] = rng.integers(0, 256, size=(int(junk.sum()), 64), dtype=np.uint8)
    d = dev(recs)
    sizes = [0, 1, 2, 63, 64, 65, 127, 255, 4097, 16385, 40000] * 27   # 297 batches > 256-slot ring
    bufs = [new_bits(n, fill=-1) for n in sizes]
    torch.cuda.synchronize()
    outs = []
    for i, (n, b) in enumerate(zip(sizes, bufs)):
        off = (i * 977) % 1000
        t = ctx.service_submit(d[off:], n, b)
        outs.append((t, off, n, b))
    for t, off, n, b in outs:
        ctx.service_wait(t, 20000)
    for t, off, n, b in outs:
        if n == 0:
            continue
        want = orc.verify_records(recs[off:off + n], hk, valid, keysel)
        got = bits_np(b, n)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (t, off, n, bad[:8], got[bad[:4]], want[bad[:4]])


def test_service_matches_launch_path_full_size(ctx):
    """2^20 and 2^24 records: service verdicts == launch-path verdicts == generator truth."""
    ctx.key_add(0, orc.KEY_1111)
    for n in (1 << 20, 1 << 24):
        recs = torch.empty((n, 64), dtype=torch.uint8, device=DEV)
        ctx.gen_records(recs, n, orc.SEED_RECORDS)
        a = new_bits(n)
        ctx.verify_records(recs, n, a)
        b = new_bits(n, fill=-1)
        torch.cuda.synchronize()
        tickets = [ctx.service_submit(recs, n, b) for _ in range(3)]
        ctx.service_wait(tickets[-1], 20000)
        assert torch.equal(a, b)
        got = hfv.bits_to_bool(bits_np(b, n), n)
        assert np.array_equal(got, orc.expected_pass_rule(n))
        ctx.service_stop()
        del recs


def test_service_sees_rewritten_records(ctx):
    """A batch buffer rewritten between batches (as an RX ring is) is read fresh: the grid
    drops stale cache lines when it picks up a descriptor."""
    ctx.key_add(0, orc.KEY_1111)
    hk, valid = orc.key_table(orc.KEY_1111)
    n = 200_000
    a = orc.gen_records(n, hk, 0, seed=1)
    b = orc.gen_records(n, hk, 0, seed=2)
    d = dev(a)
    bits = new_bits(n)
    torch.cuda.synchronize()
    t = ctx.service_submit(d, n, bits)
    ctx.service_wait(t, 20000)
    assert np.array_equal(bits_np(bits, n), orc.verify_records(a, hk, valid, 0))
    d.copy_(torch.from_numpy(b).to(DEV))
    torch.cuda.synchronize()
    t = ctx.service_submit(d, n, bits)
    ctx.service_wait(t, 20000)
    assert np.array_equal(bits_np(bits, n), orc.verify_records(b, hk, valid, 0))


@pytest.mark.parametrize("keysel", [0, 1])
def test_service_key_change_is_a_batch_boundary(ctx, keysel):
    """Key add/remove while the service runs apply from the next submitted batch on; the
    batches posted before keep the old table.  keysel 1: whole 256-key tables change (the three-table
    corpus of tests/key_tables.py), which the service kernel reads from the device table; slot 0's
    key alone travels in its kernel arguments."""
    if keysel:
        ctx.set_keysel(hfv.KEYSEL_IFID)
        n = KT.N
        d = dev(KT.corpus()[0])
        outs = [new_bits(n, fill=-1) for _ in range(3)]
        torch.cuda.synchronize()
        tickets = []
        for o, name in zip(outs, "ABA"):
            raw = KT.tables()[name][0]
            for k in range(256):
                ctx.key_add(k, raw[16 * k:16 * k + 16])
            tickets.append(ctx.service_submit(d, n, o))
        for t in tickets:
            ctx.service_wait(t, 20000)
        for o, name in zip(outs, "ABA"):
            assert np.array_equal(bits_np(o, n), KT.want()[name]), name
        return
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    outs = [new_bits(n, fill=-1) for _ in range(3)]
    torch.cuda.synchronize()
    t0 = ctx.service_submit(d, n, outs[0])
    ctx.key_remove(0)
    t1 = ctx.service_submit(d, n, outs[1])
    ctx.key_add(0, orc.KEY_1111)
    t2 = ctx.service_submit(d, n, outs[2])
    for t in (t0, t1, t2):
        ctx.service_wait(t, 20000)
    assert np.array_equal(bits_np(outs[0], n), g["pass_bits"])
    assert not bits_np(outs[1], n).any()            # slot 0 empty: fail closed
    assert np.array_equal(bits_np(outs[2], n), g["pass_bits"])


def test_service_tickets_monotonic_across_restarts(ctx):
    """three batches, a key change (grid restart at the batch boundary), three
    more, then an explicit restart through the launch path: every ticket is distinct and
    waiting on any earlier one reports it done (not 'unknown', not an alias of a new batch)."""
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    outs = [new_bits(n, fill=-1) for _ in range(7)]
    torch.cuda.synchronize()
    ts = [ctx.service_submit(d, n, outs[i]) for i in range(3)]
    ctx.key_add(1, orc.KEY_1111)                   # key table changed: restart at the next submit
    ts += ctx.service_submitv([(d, n, outs[i]) for i in range(3, 6)])
    ctx.verify_records(d, n, outs[6])              # launch path: stops the service
    ts.append(ctx.service_submit(d, n, new_bits(n)))
    assert len(set(ts)) == len(ts) and ts == sorted(ts)
    for t in ts:
        ctx.service_wait(t, 20000)
        assert ctx.service_poll(t)
    for o in outs:
        assert np.array_equal(bits_np(o, n), g["pass_bits"])
    with pytest.raises(hfv.HfvError):
        ctx.service_wait(ts[-1] + 1)               # never issued


def test_service_submitv_golden_ifid(ctx):
    """Several batches posted by one hfv_service_submitv call, 256-key table (config 3)."""
    g = orc.load_golden("hf_ifid256.npz")
    n = len(g["records"])
    d = dev(g["records"])
    nk = int(g["nkeys"])
    raw = g["raw_keys"].reshape(-1).tobytes()[:16 * nk]
    ctx.key_add_batch(0, raw)
    ctx.set_keysel(hfv.KEYSEL_IFID)
    parts = [(0, 1), (1, 333), (333, 640), (640, n)]
    outs = [new_bits(b - a, fill=-1) for a, b in parts]
    torch.cuda.synchronize()
    ts = ctx.service_submitv([(d[a:], b - a, o) for (a, b), o in zip(parts, outs)])
    for t in ts:
        ctx.service_wait(t, 20000)
    hk, valid = orc.key_table(raw)
    for (a, b), o in zip(parts, outs):
        assert np.array_equal(bits_np(o, b - a), orc.verify_records(g["records"][a:b], hk, valid, 1))


@pytest.mark.parametrize("count", [1, 20, 300], ids=["one", "twenty", "past_ring"])
def test_service_run_async(ctx, count):
    """hfv_service_run_async: returns once the grid is launched; a device synchronize covers
    the whole run (the grid exits by itself behind its stop), bitmaps equal the oracle's, and
    service_stop reaps the grid and reports its lifetime."""
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    torch.cuda.synchronize()
    cuts = [(k * 11) % (n - 64) for k in range(count)]
    outs = [new_bits(n - c, fill=-1) for c in cuts]
    ts = ctx.service_run_async([(d[c:], n - c, o) for c, o in zip(cuts, outs)])
    assert len(ts) == count
    torch.cuda.synchronize()
    for t in ts:
        assert ctx.service_poll(t)
    hk, valid = orc.key_table(orc.KEY_1111)
    for c, o in zip(cuts, outs):
        assert np.array_equal(bits_np(o, n - c), orc.verify_records(g["records"][c:], hk, valid, 0))
    assert ctx.service_stop() > 0 and not ctx.service_running


def test_service_balance_weights_stay_bounded(ctx):
    """svc_balance (hfv_service.cpp) re-derives the per-XCD block weights after every run grid:
    over a dozen K = 20 grids of 2^20 records (the bench's shape) they stay inside the clamp
    [1/2, 2] of an equal share, and every grid's verdicts stay equal
    to the launch path's whatever the shares."""
    ctx.key_add(0, orc.KEY_1111)
    n = 1 << 20
    recs = torch.empty((n, 64), dtype=torch.uint8, device=DEV)
    ctx.gen_records(recs, n, orc.SEED_RECORDS)
    want = new_bits(n)
    ctx.verify_records(recs, n, want)
    outs = [new_bits(n, fill=-1) for _ in range(20)]
    torch.cuda.synchronize()
    for _ in range(12):
        for o in outs:
            o.fill_(-1)
        torch.cuda.synchronize()
        ctx.service_run_async([(recs, n, o) for o in outs])
        torch.cuda.synchronize()
        assert ctx.service_stop() >= 0
        for o in outs:
            assert torch.equal(o, want)
        w = ctx.service_weights()
        assert w is not None and len(w) == 9
        assert all(512 <= x <= 2048 for x in w), w   # (quiet boxes: within -10 % / +5 %, profiles/r03/slowgrid/)


@pytest.mark.parametrize("then", ["submit", "submitv", "start_submit"])
def test_service_submit_after_run_async(ctx, then):
    """after hfv_service_run_async the grid exits on its own stop; a later
    submit (or start + submit) with no service_stop in between must reap it and post to a
    fresh grid, so the new tickets complete instead of sitting in a ring nobody reads."""
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    first = [new_bits(n, fill=-1) for _ in range(3)]
    torch.cuda.synchronize()
    ts = ctx.service_run_async([(d, n, o) for o in first])
    outs = [new_bits(n, fill=-1) for _ in range(2)]
    torch.cuda.synchronize()
    if then == "submit":
        new = [ctx.service_submit(d, n, o) for o in outs]
    elif then == "submitv":
        new = ctx.service_submitv([(d, n, o) for o in outs])
    else:
        ctx.service_start()
        assert ctx.service_running
        new = [ctx.service_submit(d, n, o) for o in outs]
    assert new[0] > ts[-1]
    for t in ts + list(new):
        ctx.service_wait(t, 20000)
        assert ctx.service_poll(t) == 1
    for o in first + outs:
        assert np.array_equal(bits_np(o, n), g["pass_bits"])


@pytest.mark.parametrize("count", [1, 5, 300], ids=["one", "five", "past_ring"])
def test_service_run_one_shot(ctx, count):
    """hfv_service_run: batches + stop posted before the grid starts (a run longer than the
    ring launches once it is full); every ticket is done on return, bitmaps equal the
    oracle's, and the ctx serves a later submit on a new grid."""
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    torch.cuda.synchronize()
    cuts = [(k * 7) % (n - 64) for k in range(count)]
    outs = [new_bits(n - c, fill=-1) for c in cuts]
    ts, ms = ctx.service_run([(d[c:], n - c, o) for c, o in zip(cuts, outs)])
    assert len(ts) == count and ms > 0 and not ctx.service_running
    for t in ts:
        assert ctx.service_poll(t)
    hk, valid = orc.key_table(orc.KEY_1111)
    for c, o in zip(cuts, outs):
        assert np.array_equal(bits_np(o, n - c), orc.verify_records(g["records"][c:], hk, valid, 0))
    bits = new_bits(n, fill=-1)
    t = ctx.service_submit(d, n, bits)
    ctx.service_wait(t, 20000)
    assert np.array_equal(bits_np(bits, n), g["pass_bits"])
    assert ts[-1] < t
    ctx.service_stop()


def test_service_no_key_fails_closed(ctx):
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    bits = new_bits(n, fill=-1)
    d = dev(g["records"])
    torch.cuda.synchronize()
    t = ctx.service_submit(d, n, bits)
    ctx.service_wait(t, 20000)
    assert not bits_np(bits, n).any()


def test_service_coexists_with_launch_path(ctx):
    """A launch-path call stops the service at a batch boundary; the next submit restarts it."""
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    b1, b2, b3 = new_bits(n, -1), new_bits(n, -1), new_bits(n, -1)
    torch.cuda.synchronize()
    t = ctx.service_submit(d, n, b1)
    ctx.verify_records(d, n, b2)
    assert not ctx.service_running
    ctx.service_wait(t, 1000)                      # completed before the stop
    t = ctx.service_submit(d, n, b3)
    assert ctx.service_running
    ctx.service_wait(t, 20000)
    for b in (b1, b2, b3):
        assert np.array_equal(bits_np(b, n), g["pass_bits"])


def test_service_idle_exit_and_restart(ctx):
    """The grid leaves by itself after idle_ms without work; the next submit starts a new one."""
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    ctx.service_start(idle_ms=50)
    b = new_bits(n, -1)
    b2 = new_bits(n, -1)
    torch.cuda.synchronize()
    t = ctx.service_submit(d, n, b)
    ctx.service_wait(t, 20000)
    time.sleep(0.5)                                # > idle_ms: the grid has exited
    t = ctx.service_submit(d, n, b2)               # restarts it
    ctx.service_wait(t, 20000)
    assert np.array_equal(bits_np(b2, n), g["pass_bits"])


def test_service_poll_after_idle_exit(ctx):
    """a grid whose relay wave leaves on the idle timeout while its blocks
    still work through earlier batches forwards no more completions to the host ring.  The
    batches here all travel in the kernel arguments, so the idle timer runs from grid start, and
    they take longer than idle_ms.  hfv_service_poll alone must still see every ticket complete
    (it reaps the exited grid and reads the device completion words) instead of 0 forever."""
    ctx.key_add(0, orc.KEY_1111)
    n, K = 1 << 22, 40                             # ~45 us of work per batch: ~1.8 ms > idle_ms
    recs = torch.empty((n, 64), dtype=torch.uint8, device=DEV)
    ctx.gen_records(recs, n, orc.SEED_RECORDS)
    want = new_bits(n)
    ctx.verify_records(recs, n, want)
    ctx.service_start(idle_ms=1)                   # later grids keep the 1 ms idle timeout
    ctx.service_stop()
    outs = [new_bits(n, fill=-1) for _ in range(K)]
    torch.cuda.synchronize()
    tickets = ctx.service_submitv([(recs, n, o) for o in outs])
    done, t_end = set(), time.time() + 30
    while len(done) < K and time.time() < t_end:
        for t in tickets:
            if t not in done and ctx.service_poll(t):
                done.add(t)
    assert len(done) == K, f"{K - len(done)} tickets never reported done by polling"
    for i, o in enumerate(outs):
        assert torch.equal(o, want), f"batch {i}"


def test_service_bad_arguments(ctx):
    ctx.key_add(0, orc.KEY_1111)
    bits = new_bits(4)
    recs = torch.zeros((4, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(hfv.HfvError):
        ctx.service_submit(recs.data_ptr() + 4, 3, bits)
    with pytest.raises(hfv.HfvError):
        ctx.service_submit(recs, 4, bits, stride=40)
    with pytest.raises(hfv.HfvError):
        ctx.service_wait(12345)


def _grid_ms(ctx, posts):
    """One hfv_service_run_async grid over the prepared batches; its event-timed lifetime."""
    ctx.service_set_timing(True)
    ctx.service_run_async(posts)
    torch.cuda.synchronize()
    return ctx.service_stop()


@pytest.mark.parametrize("k,n", [(20, 1 << 20), (100, 1 << 18)], ids=["k20_2e20", "k100_2e18"])
def test_service_grid_ignores_host_round_trips(request, ctx, k, n):
    """the resident grid must not run at the pace of host-memory round trips.
    A debug hook makes every host read of the relay wave take 30 us longer (a slow PCIe link,
    as on the driver's round-3 box, whose service grids ran at ~42 us per 2^20 batch).  K = 20
    batches all travel in the kernel arguments; K = 100 puts 36 behind the relay's read-ahead.
    Either way no block ever waits for a descriptor, the verdicts equal the launch path's, and
    the delayed grids stay within 1.5x of the undelayed ones (within noise in practice)."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    ctx.key_add(0, orc.KEY_1111)
    R = 4
    recs = [torch.empty((n, 64), dtype=torch.uint8, device=DEV) for _ in range(R)]
    want = []
    for i, r in enumerate(recs):
        ctx.gen_records(r, n, orc.SEED_RECORDS, first_index=i * n)
        w = new_bits(n)
        ctx.verify_records(r, n, w)
        want.append(w)
    outs = [new_bits(n, fill=-1) for _ in range(k)]
    torch.cuda.synchronize()
    posts = ctx.service_batches([(recs[i % R], n, outs[i]) for i in range(k)])
    times = {0: [], 30: []}
    cycles = {0: [], 30: []}   # grid time x block 0's shader clock: the clock-independent check
    try:
        _grid_ms(ctx, posts)   # warm-up grid
        for _ in range(3):
            for us in (0, 30):
                hfv.Ctx.debug_relay_delay(us)
                for o in outs:
                    o.fill_(-1)
                torch.cuda.synchronize()
                times[us].append(_grid_ms(ctx, posts))
                mhz = ctx.service_shader_mhz()
                if mhz:
                    cycles[us].append(times[us][-1] * 1e3 * mhz)
                rel = ctx.service_relay()
                assert rel["block_waits"] == 0, rel
                assert rel["inline"] == min(k + 1, hfv.SVC_INLINE), rel
                assert rel["relayed"] == max(0, k + 1 - hfv.SVC_INLINE), rel
                if us:   # the hook really delayed the host reads (the probe at grid start, and the relay's)
                    assert rel["probe_rtt_us"] >= us, rel
                    if k + 1 > hfv.SVC_INLINE:
                        assert rel["host_reads"] > 0 and rel["read_rtt_max_us"] >= us, rel
                if k + 1 <= hfv.SVC_INLINE:
                    assert rel["host_reads"] == 0, rel   # every batch and the stop were inline
                for i, o in enumerate(outs):
                    assert torch.equal(o, want[i % R]), f"batch {i}"
    finally:
        hfv.Ctx.debug_relay_delay(0)
    fast, slow = sorted(times[0])[1], sorted(times[30])[1]
    print(f"K={k} n={n}: grids {times}, medians {fast:.4f} / {slow:.4f} ms")
    # the deterministic proof is above (no block waited, every descriptor inline or read ahead);
    # the timing bound is loose (clocks vary on a shared box) but still catches a grid
    # at the pace of the delayed round trips (round 3's fault: 3-4x)
    assert slow <= 1.5 * fast, times
    # the same comparison in shader cycles (the box's clock varies from grid to grid,
    # the work per cycle does not), so a regression well below 1.5x is caught too
    if len(cycles[0]) == 3 and len(cycles[30]) == 3:
        cf, cs = sorted(cycles[0])[1], sorted(cycles[30])[1]
        assert cs <= 1.2 * cf, cycles


def test_service_live_submits_with_slow_host_link(request, ctx):
    """The relay's other duties under a slow host link (30 us extra per host read): descriptors
    posted one at a time to a running grid, and completions forwarded to the host ring so that
    hfv_service_wait and ring-slot reuse (more batches than ring slots) still work."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    g = orc.load_golden("hf_single.npz")
    n = len(g["records"])
    d = dev(g["records"])
    ctx.key_add(0, orc.KEY_1111)
    hk, valid = orc.key_table(orc.KEY_1111)
    want = orc.verify_records(g["records"], hk, valid, 0)
    try:
        hfv.Ctx.debug_relay_delay(30)
        outs = [new_bits(n, fill=-1) for _ in range(hfv.SVC_RING + 40)]
        torch.cuda.synchronize()
        ctx.service_start()
        ts = []
        for i, o in enumerate(outs):
            ts.append(ctx.service_submit(d, n, o))
            if i % 50 == 0:
                ctx.service_wait(ts[-1], 20000)    # a forwarded completion while the grid runs
                assert ctx.service_poll(ts[-1])
        ctx.service_wait(ts[-1], 20000)
        for o in outs:
            assert np.array_equal(bits_np(o, n), want)
        ctx.service_stop()
        rel = ctx.service_relay()
        assert rel["relayed"] >= len(outs) and rel["forwarded"] >= hfv.SVC_RING, rel
    finally:
        hfv.Ctx.debug_relay_delay(0)


@pytest.mark.parametrize("k", [3, 6, 9])
def test_service_run_ragged_large_batches(ctx, k):
    """Run grids of large ragged batches (a partial last tile, block shares that end mid-tile),
    back to back (the per-grid scratch alternates): verdicts equal to the launch path's for
    every batch, no block waits for a descriptor, nothing relayed (all inline)."""
    ctx.key_add(0, orc.KEY_1111)
    base = 1 << 19
    sizes = [base + 37 * i + (i % 3) for i in range(k)]
    recs = torch.empty((max(sizes), 64), dtype=torch.uint8, device=DEV)
    ctx.gen_records(recs, max(sizes), orc.SEED_RECORDS)
    want = []
    for n in sizes:
        w = new_bits(n)
        ctx.verify_records(recs, n, w)
        want.append(w)
    outs = [new_bits(n, fill=-1) for n in sizes]
    torch.cuda.synchronize()
    for _ in range(3):
        for o in outs:
            o.fill_(-1)
        torch.cuda.synchronize()
        ts = ctx.service_run_async([(recs, n, o) for n, o in zip(sizes, outs)])
        torch.cuda.synchronize()
        for t in ts:
            assert ctx.service_poll(t)
        assert ctx.service_stop() > 0
        for i, (o, w) in enumerate(zip(outs, want)):
            assert torch.equal(o, w), f"batch {i}"
    rel = ctx.service_relay()
    assert rel["block_waits"] == 0 and rel["relayed"] == 0, rel


@pytest.mark.parametrize("keysel", [0, 1])
def test_service_soak_random_shapes(ctx, keysel):
    """A short soak (scripts/svc_soak.py runs the long form): grids of random shape -- K from 1
    to 300 (inline, relayed, past the ring), batch sizes from 1 to 2^18 records at random
    64-aligned offsets, through hfv_service_run, run_async and live submits in bursts -- for a
    few seconds; every bitmap must equal the launch path's over the same records."""
    import random
    rng = random.Random(11 + keysel)
    n_all = 1 << 19
    recs = torch.empty((n_all, 64), dtype=torch.uint8, device=DEV)
    if keysel:
        ctx.key_add_batch(0, bytes(rng.randrange(256) for _ in range(256 * 16)))   # 256 interface keys
        ctx.set_keysel(hfv.KEYSEL_IFID)
    else:
        ctx.key_add(0, orc.KEY_1111)
    ctx.gen_records(recs, n_all, 0x5C100001, first_index=0)
    ref = new_bits(n_all)
    ctx.verify_records(recs, n_all, ref)
    ref_bits = np.unpackbits(bits_np(ref, n_all).view(np.uint8), bitorder="little")
    grids = 0
    t_end = time.time() + 4.0
    while time.time() < t_end:
        k = rng.choice([1, 2, 20, 64, 65, 300])
        shape = []
        for _ in range(k):
            n = rng.choice([1, 63, 64, 65, 1000, 65536, 1 << 18])
            shape.append(((rng.randrange(0, n_all - n + 1) & ~63), n))
        outs = [new_bits(n, fill=-1) for _, n in shape]
        specs = [(recs[off:off + n], n, o) for (off, n), o in zip(shape, outs)]
        torch.cuda.synchronize()
        mode = rng.choice(["run", "async", "live"])
        if mode == "run":
            ctx.service_run(specs)
        elif mode == "async":
            ctx.service_run_async(specs)
            torch.cuda.synchronize()
            ctx.service_stop()
        else:
            ts = []
            for i in range(0, len(specs), 7):
                ts += ctx.service_submitv(specs[i:i + 7])
            for t in ts:
                ctx.service_wait(t, 20000)
            ctx.service_stop()
        for (off, n), o in zip(shape, outs):
            want = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
            want[:n] = ref_bits[off:off + n]
            assert np.array_equal(bits_np(o, n), np.packbits(want, bitorder="little").view(np.uint64)), \
                (grids, mode, k, off, n)
        grids += 1
    assert grids >= 10
