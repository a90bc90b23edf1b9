"""Key-table publication (publish_keys / note_reader in csrc/hfv_publish.cpp) held on the kernels that
read the device table: a launch verifies under the table it was launched with, whatever the host
installs afterwards and on whichever stream.

Under KEYSEL_ZERO the verify kernels take slot 0's key from their kernel arguments and never read
the device table, so every test here runs per-interface keys (KEYSEL_IFID, or a key_index array)
over the corpus of tests/key_tables.py: three 256-key tables A, B, C and 4500 records of which
each table passes only its own third.  A launch that read another table than its own differs from
the oracle in well over half of its bits.  The router test does the same with the router tables,
which are published in the same device image.

Every race is made by torch.cuda._sleep on the slow side's stream, with every buffer and stream
created before it and only key_add / br_set_config (host shadow only) inside it.  An event recorded
behind the slow launch must still be pending once the host has enqueued the racing work
(Window.assert_open): a test whose window had closed fails instead of passing.  Each test prints
the sleep's duration and the host time it had to cover (pytest -s).

What holds which part of the mechanism (shown by running this file against the A/B builds
`make nofence` and `make noreaderfence` through HFV_LIB; both must fail, with wrong verdicts):
  read-after-write fence (pub_pending / img_free):  test_read_after_write_across_streams, test_frames_read_after_write
  write-after-read fence (reader_ev):  test_write_after_read_across_streams[caller-*], test_service_*, test_router_tables_*
  own-stream branch:                   test_write_after_read_across_streams[own-*]
  overflow path (hipDeviceSynchronize): test_reader_overflow
  staging image reuse (host wait):     test_same_stream_order
Integer work: every comparison is bit-exact against the CPU checker."""
import ctypes
import time

import numpy as np
import pytest

import br_fuzz as F
import br_topo as T
import key_tables as KT
import orc
import scion_hfv as hfv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = KT.N
# torch.cuda._sleep spins on the shader clock: 20M cycles measured 8.3-9.6 ms on an MI355X, against
# 0.05-0.4 ms of host work per window (two tables of 256 key_add calls and up to a dozen launches)
SLEEP_CYCLES = 20_000_000
MAC = lambda k, m: orc.cmac(m, k)   # noqa: E731  checker-side AES for building test paths


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def host(t):
    return t.cpu().numpy()


def new_bits(n):
    return torch.zeros(max(1, (n + 63) // 64), dtype=torch.int64, device=DEV)


_KEYS = {}


def install(ctx, name):
    """Table `name` into the host shadow table: key_add only (no device work, no synchronize)."""
    if name not in _KEYS:
        raw = KT.tables()[name][0]
        _KEYS[name] = [raw[16 * k:16 * k + 16] for k in range(256)]
    for k, key in enumerate(_KEYS[name]):
        ctx.key_add(k, key)


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    c.set_keysel(hfv.KEYSEL_IFID)
    yield c
    torch.cuda.synchronize()
    c.service_stop()
    c.synchronize()
    c.close()


class Window:
    """The race window: a sleep on `stream`, an event behind the slow launch that follows it, and
    the assertion that this event is still pending after the host enqueued the racing work."""

    def __init__(self, stream):
        self.stream = stream
        self.t0 = torch.cuda.Event(enable_timing=True)
        self.t1 = torch.cuda.Event(enable_timing=True)
        self.done = torch.cuda.Event()
        for e in (self.t0, self.t1, self.done):   # events are created on their first record: do it now
            e.record(stream)
        self.host_ms = None

    def open(self):
        torch.cuda.synchronize()
        self.t0.record(self.stream)
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(SLEEP_CYCLES)
        self.t1.record(self.stream)
        self.host0 = time.perf_counter()

    def mark(self):
        """Behind the slow launch."""
        self.done.record(self.stream)

    def assert_open(self):
        pending = not self.done.query()
        self.host_ms = (time.perf_counter() - self.host0) * 1e3
        assert pending, "the slow launch finished before the racing work was enqueued (%.2f ms of host work): " \
                        "the race was not exercised" % self.host_ms

    def report(self, what):
        torch.cuda.synchronize()
        print("\n%s: window open; sleep %.2f ms (%d cycles), host enqueue %.2f ms"
              % (what, self.t0.elapsed_time(self.t1), SLEEP_CYCLES, self.host_ms))


PROBE_CYCLES = 2_000_000   # under a millisecond


def concurrent_with(slow, tries=16):
    """A torch stream whose work runs while `slow` is busy.  HIP maps its streams onto a few
    hardware queues (four by default) and two streams on one queue run in order: the racing side
    would then sit behind the sleep, the host would wait for its publish copy until the sleep is
    over, and no race would take place.  Each candidate from torch's pool is probed: a small
    kernel on it must finish while a short sleep on `slow` is still running."""
    flag = torch.zeros(1, device=DEV)
    e_slow, e = torch.cuda.Event(), torch.cuda.Event()
    for _ in range(tries):
        s = torch.cuda.Stream()
        if s.cuda_stream == slow.cuda_stream:
            continue
        torch.cuda.synchronize()
        with torch.cuda.stream(slow):
            torch.cuda._sleep(PROBE_CYCLES)
        e_slow.record(slow)
        with torch.cuda.stream(s):
            flag.add_(1)
        e.record(s)
        e.synchronize()
        overlapped = not e_slow.query()
        torch.cuda.synchronize()
        if overlapped:
            return s
    pytest.fail("no stream of torch's pool runs concurrently with the slow stream")


# ---- readers of the device key table ----------------------------------------------------------

class Records:
    """verify_records under KEYSEL_IFID (k_verify_records<IFID>)"""

    def __init__(self):
        self.d = dev(KT.corpus()[0])

    def out(self):
        return new_bits(N)

    def launch(self, ctx, out, stream):
        ctx.verify_records(self.d, N, out, stream=stream)

    def check(self, out, name):
        assert np.array_equal(host(out).view(np.uint64), KT.want()[name]), "verdicts are not table %s's" % name


class Batches(Records):
    """verify_batches under KEYSEL_IFID (k_verify_batches<IFID>): the corpus cut at KT.CUTS"""

    def out(self):
        spans = list(zip(KT.CUTS[:-1], KT.CUTS[1:]))
        bits = [new_bits(b - a) for a, b in spans]
        arr = hfv.Ctx.service_batches([(self.d.data_ptr() + 64 * a, b - a, t) for (a, b), t in zip(spans, bits)])
        return bits, arr

    def launch(self, ctx, out, stream):
        ctx.verify_batches(out[1], stream=stream)

    def check(self, out, name):
        for k, (t, want) in enumerate(zip(out[0], KT.want_batches()[name])):
            if len(want):
                assert np.array_equal(host(t).view(np.uint64), want), "batch %d: verdicts are not table %s's" % (k, name)


class Macinputs:
    """verify_macinputs with a key_index array (k_macinputs: fill_keys)"""

    def __init__(self):
        mi, expected, kidx = KT.macinputs()
        self.mi, self.expected, self.kidx = dev(mi), dev(expected.view(np.int64)), dev(kidx)

    def out(self):
        return new_bits(N)

    def launch(self, ctx, out, stream):
        ctx.verify_macinputs(self.mi, self.expected, N, out, key_index=self.kidx, stream=stream)

    def check(self, out, name):
        assert np.array_equal(host(out).view(np.uint64), KT.want()[name]), "verdicts are not table %s's" % name


class Tags(Macinputs):
    """cmac_tags with a key_index array: full 16-byte tags of a 256-record sample"""

    def out(self):
        return torch.zeros((N, 16), dtype=torch.uint8, device=DEV)

    def launch(self, ctx, out, stream):
        ctx.cmac_tags(self.mi, N, out, key_index=self.kidx, stream=stream)

    def check(self, out, name):
        assert np.array_equal(host(out)[KT.tag_sample()], KT.want_tags()[name]), "tags are not table %s's" % name


class Generator:
    """gen_records under KEYSEL_IFID (k_gen_records): the bytes carry MACs under the table's keys"""

    def out(self):
        return torch.zeros((KT.GEN_N, 64), dtype=torch.uint8, device=DEV)

    def launch(self, ctx, out, stream):
        ctx.gen_records(out, KT.GEN_N, orc.SEED_RECORDS, stream=stream)

    def check(self, out, name):
        assert np.array_equal(host(out), KT.want_gen()[name]), "records are not generated under table %s" % name


READERS = [Records, Batches, Macinputs, Tags, Generator]
readers = pytest.mark.parametrize("reader", READERS, ids=lambda r: r.__name__.lower())


# ---- the tests -------------------------------------------------------------------------------

@readers
def test_same_stream_order(ctx, reader):
    """One stream, behind a sleep: launch under A, install B, launch, install C, launch.  The third
    publish overwrites the device table A's launch reads, and each publish rewrites the one pinned
    staging image the previous copy is read from.  A is published by a warm-up, so that the window
    assertion can be made after B's launch was enqueued: a second publish inside one window waits
    on the host for the first one's copy, that is for the sleep."""
    r = reader()
    s = torch.cuda.Stream()
    outs = [r.out() for _ in range(4)]
    w = Window(s)
    install(ctx, "A")
    r.launch(ctx, outs[3], s)
    w.open()
    r.launch(ctx, outs[0], s)
    w.mark()
    install(ctx, "B")
    r.launch(ctx, outs[1], s)
    w.assert_open()
    install(ctx, "C")
    r.launch(ctx, outs[2], s)
    w.report("same stream")
    for o, name in zip(outs, "ABCA"):
        r.check(o, name)


@readers
def test_read_after_write_across_streams(ctx, reader):
    """Both device tables hold a wrong table (B, C); A's publish copy is queued behind a sleep on
    stream a.  Launches on stream b and on the NULL stream must wait for that copy."""
    r = reader()
    a = torch.cuda.Stream()
    b = concurrent_with(a)
    outs = [r.out() for _ in range(4)]
    w = Window(a)
    for wrong in "BC":
        install(ctx, wrong)
        r.launch(ctx, outs[3], a)
        torch.cuda.synchronize()
        r.check(outs[3], wrong)
    install(ctx, "A")
    w.open()
    r.launch(ctx, outs[0], a)       # publishes: the copy waits behind the sleep
    w.mark()
    r.launch(ctx, outs[1], b)
    r.launch(ctx, outs[2], 0)
    w.assert_open()
    w.report("read after write")
    for o in outs[:3]:
        r.check(o, "A")


def _slow_stream(ctx, own):
    return torch.cuda.ExternalStream(ctx.stream) if own else torch.cuda.Stream()


@readers
@pytest.mark.parametrize("own", [False, True], ids=["caller", "own"])
def test_write_after_read_across_streams(ctx, reader, own):
    """S1 launches under A behind a sleep without publishing (it reads device table X).  On S2,
    B is published into table Y and C into X: that copy must wait for S1's launch.  With `own`,
    S1 is the ctx's own stream, whose fence event is recorded at publish time."""
    r = reader()
    s1 = _slow_stream(ctx, own)
    s2 = concurrent_with(s1)
    outs = [r.out() for _ in range(4)]
    w = Window(s1)
    install(ctx, "A")
    r.launch(ctx, outs[3], s2)       # warm-up: A is in table X
    w.open()
    r.launch(ctx, outs[0], s1)
    w.mark()
    install(ctx, "B")
    r.launch(ctx, outs[1], s2)
    install(ctx, "C")
    r.launch(ctx, outs[2], s2)
    w.assert_open()
    w.report("write after read (%s stream)" % ("own" if own else "caller"))
    for o, name in zip(outs, "ABCA"):
        r.check(o, name)


@readers
@pytest.mark.parametrize("slow", [9, 0], ids=["tenth-slow", "first-slow"])
def test_reader_overflow(ctx, reader, slow):
    """Ten caller streams launch under A (the table keeps eight reader slots), one of them behind a
    sleep; B and C are published on an eleventh.  C's publish overwrites the table all ten read."""
    r = reader()
    streams = [torch.cuda.Stream() for _ in range(10)]
    p = concurrent_with(streams[slow])
    for _ in range(16):              # torch's pool hands its streams out in turn: an eleventh one
        if p.cuda_stream not in {s.cuda_stream for s in streams}:
            break
        p = concurrent_with(streams[slow])
    assert len({s.cuda_stream for s in streams + [p]}) == 11
    outs = [r.out() for _ in range(10)]
    warm, out_b, out_c = r.out(), r.out(), r.out()
    w = Window(streams[slow])
    install(ctx, "A")
    r.launch(ctx, warm, p)
    w.open()
    for i, s in enumerate(streams):
        r.launch(ctx, outs[i], s)
        if i == slow:
            w.mark()
    install(ctx, "B")
    r.launch(ctx, out_b, p)
    install(ctx, "C")
    w.assert_open()                 # the publish below waits for the device on the host
    r.launch(ctx, out_c, p)
    w.report("reader overflow (stream %d slow)" % slow)
    for o in outs:
        r.check(o, "A")
    r.check(out_b, "B")
    r.check(out_c, "C")


@readers
def test_table_update_after_reader_stream_destroyed(ctx, reader):
    """A table change after the stream that last read the table was destroyed (hipStreamDestroy,
    not a pooled torch stream): the publish fences on the event recorded behind that stream's
    launch, never on the dead stream."""
    L = hfv.lib()   # the HIP runtime the library itself is linked against
    create, destroy, sync = L.hipStreamCreateWithFlags, L.hipStreamDestroy, L.hipStreamSynchronize
    create.argtypes, create.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], ctypes.c_int
    for f in (destroy, sync):
        f.argtypes, f.restype = [ctypes.c_void_p], ctypes.c_int
    r = reader()
    torch.cuda.synchronize()
    for name in "ABCAB":
        install(ctx, name)
        s = ctypes.c_void_p()
        assert create(ctypes.byref(s), 1) == 0 and s.value        # hipStreamNonBlocking
        out = r.out()
        torch.cuda.synchronize()
        r.launch(ctx, out, s.value)
        assert sync(s) == 0
        r.check(out, name)
        assert destroy(s) == 0
    install(ctx, "C")
    out = r.out()
    torch.cuda.synchronize()
    r.launch(ctx, out, torch.cuda.Stream())
    torch.cuda.synchronize()
    r.check(out, "C")


def test_service_restart_waits_for_a_slow_reader(ctx):
    """S1 runs verify_records under A behind a sleep; the resident service then verifies a batch
    under B and, restarted at the key change, one under C.  The restart publishes C into the table
    S1's launch reads and must wait for it."""
    r = Records()
    outs = [r.out() for _ in range(4)]
    install(ctx, "A")
    torch.cuda.synchronize()
    t = ctx.service_submit(r.d, N, outs[3])      # warm-up: A published, the service's buffers exist
    ctx.service_wait(t, 20000)
    ctx.service_stop()
    r.check(outs[3], "A")
    # S1: a stream beside which the service's own stream runs (see concurrent_with)
    probe = torch.cuda.Event()
    for _ in range(16):
        s1 = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            torch.cuda._sleep(5 * PROBE_CYCLES)
        probe.record(s1)
        t = ctx.service_submit(r.d, N, outs[3])
        ctx.service_wait(t, 20000)
        overlapped = not probe.query()
        ctx.service_stop()
        torch.cuda.synchronize()
        if overlapped:
            break
    else:
        pytest.fail("the service ran beside no stream of torch's pool")
    w = Window(s1)
    w.open()
    r.launch(ctx, outs[0], s1)
    w.mark()
    install(ctx, "B")
    t = ctx.service_submit(r.d, N, outs[1])
    ctx.service_wait(t, 20000)
    install(ctx, "C")
    t = ctx.service_submit(r.d, N, outs[2])
    w.assert_open()
    ctx.service_wait(t, 20000)
    ctx.service_stop()
    s1.synchronize()
    w.report("service")
    for o, name in zip(outs[:3], "ABC"):
        r.check(o, name)


_BR = {}


def _router_cases():
    """1024 frames (br_fuzz.fuzz_batch for br1, br2 and br3, a third each) and three (router tables, slot-0 key) pairs with the
    oracle router's results under each, built once."""
    if not _BR:
        brs = {b: T.OracleBR(T.br_config(b, False)) for b in ("br1", "br2", "br3")}
        hops = F.hop_inputs(brs, False, MAC)
        parts = [F.fuzz_batch(hops, br, False, k, seed=400 + i, slot=F.TABLE_FUZZ_SLOT)
                 for i, (br, k) in enumerate((("br1", 342), ("br2", 341), ("br3", 341)))]
        frames, lens, ifidx = (np.concatenate([p[j] for p in parts]) for j in range(3))
        cases = []
        for br, key in (("br1", T.KEYS[1]), ("br2", T.KEYS[1]), ("br3", T.KEYS[5])):
            cfg = T.br_config(br, False)
            ref = frames.copy()
            res = orc.br_process(ref, lens, ifidx, cfg, orc.hop_key(key))
            cases.append((cfg, key, res, ref))
        _BR["v"] = (frames, lens, ifidx, cases)
    return _BR["v"]


def _br_differ(x, y):
    (_, _, (xa, xv, xe, _), xf), (_, _, (ya, yv, ye, _), yf) = x, y
    return int(((xa != ya) | (xv != yv) | (xe != ye) | (xf != yf).any(axis=1)).sum())


def test_router_tables_write_after_read(ctx):
    """br_process (k_br_process reads keys and router tables from the same device image): a slow
    launch on S1 under br1's tables, then br2's and br3's tables (and another slot-0 key) published
    on S2, the second over the image S1 reads.  Each launch's actions, verdicts, egress, counters
    and frame bytes equal the oracle router's under that launch's own tables."""
    frames, lens, ifidx, cases = _router_cases()
    n, slot = frames.shape
    assert n == 1024
    for x in range(3):      # the three table sets give different results for whole tiles of frames
        for y in range(x + 1, 3):
            assert _br_differ(cases[x], cases[y]) >= 256, (x, y)
    ctx.set_keysel(hfv.KEYSEL_ZERO)
    dl = dev(lens.view(np.int16))
    di = dev(ifidx.view(np.int32))
    bufs = [(dev(frames), torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
             torch.zeros(n, dtype=torch.int32, device=DEV),
             torch.zeros(hfv.BR_STATS_IFINDEX * 2 * hfv.BR_COUNTERS, dtype=torch.int64, device=DEV)) for _ in range(4)]
    s1 = torch.cuda.Stream()
    s2 = concurrent_with(s1)
    w = Window(s1)

    def launch(k, stream):
        d, a, v, e, st = bufs[k]
        ctx.br_process(d, slot, dl, di, n, a, v, e, st, stream=stream)

    ctx.key_add(0, cases[0][1])
    ctx.br_set_config(cases[0][0])
    launch(3, s2)                    # warm-up: br1's tables are in image X
    w.open()
    launch(0, s1)
    w.mark()
    ctx.br_set_config(cases[1][0])
    launch(1, s2)
    ctx.br_set_config(cases[2][0])
    ctx.key_add(0, cases[2][1])
    launch(2, s2)
    w.assert_open()
    w.report("router tables")
    for k, c in ((0, 0), (1, 1), (2, 2), (3, 0)):
        d, a, v, e, st = bufs[k]
        _, _, want, ref = cases[c]
        got = (host(a), host(v), host(e), host(st).view(np.uint64))
        orc.assert_br_equal(got, host(d), want, ref, "launch %d under table set %d" % (k, c))


def test_frames_read_after_write(ctx):
    """verify_frames under KEYSEL_IFID (extract, k_verify_batches<IFID>, mask): both device tables
    hold a table whose slots 1-6 carry a wrong key; the table of
    test_verify_frames_keysel_ifid_256_keys is published behind a sleep on stream a, and a launch on
    stream b must wait for that copy."""
    import test_gpu_frames as TF
    n = 4096
    frames, lens, _ = TF.fuzz("br1", True, n, 341)
    right = bytearray(orc.gen_key_table(256))
    for ifid in range(1, 7):
        right[16 * ifid:16 * ifid + 16] = T.KEYS[1]
    right = bytes(right)
    hk, valid = orc.key_table(right)
    want, want_st = TF.oracle_bits(frames, lens, n, hk, valid, hfv.KEYSEL_IFID)
    assert int(np.unpackbits(want.view(np.uint8)).sum()) > 500
    d, dl = dev(frames), TF.dev_lens(lens)
    slot = frames.shape[1]
    bufs = [(torch.zeros((n, 64), dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
             new_bits(n)) for _ in range(3)]
    a = torch.cuda.Stream()
    b = concurrent_with(a)
    w = Window(a)

    def launch(k, stream):
        recs, status, bits = bufs[k]
        ctx.verify_frames(d, slot, dl, n, recs, status, bits, stride=64, stream=stream)

    def put(raw):
        for k in range(256):
            ctx.key_add(k, raw[16 * k:16 * k + 16])

    for wrong in (orc.gen_key_table(256), orc.gen_key_table(256, orc.SEED_KEYS + 1)):
        put(wrong)
        launch(2, a)
        torch.cuda.synchronize()
        whk, wvalid = orc.key_table(wrong)
        wbits, _ = TF.oracle_bits(frames, lens, n, whk, wvalid, hfv.KEYSEL_IFID)
        assert not wbits.any()                   # slots 1-6 hold no key these frames verify under
        assert np.array_equal(host(bufs[2][2]).view(np.uint64), wbits)
    put(right)
    w.open()
    launch(0, a)
    w.mark()
    launch(1, b)
    w.assert_open()
    w.report("frames read after write")
    for k in (0, 1):
        assert np.array_equal(host(bufs[k][1]), want_st)
        assert np.array_equal(host(bufs[k][2]).view(np.uint64), want), "stream %s" % "ab"[k]
