"""The sibling of tests/test_gpu_key_publish.py for the launches that read NO device table.

Under KEYSEL_ZERO the record and batch-list verify kernels take T0 and slot 0's key rows from their
kernel arguments and never dereference the device table they are handed, so the library does not
book such a launch as a reader of it (launch_reads_tables in csrc/hfv_ctx.h): its stream neither
waits for a publish copy pending on another stream nor leaves a fence event behind.  That predicate
MUST TRACK WHAT THE KERNELS READ: a KEYSEL_ZERO verify kernel that starts reading the table has to
flip it, or (a) below goes wrong.  What must hold all the same:

  (a) the key travels by value: a launch verifies under the slot-0 key installed when it was
      enqueued, on whichever stream, however late its stream gets to run it;
  (b) a caller stream that only ever ran such launches leaves nothing behind when it is destroyed;
  (c) a stream that did read a table (KEYSEL_IFID) is still fenced when KEYSEL_ZERO launches and
      key changes come between its launch and the publish that overwrites its table.

1029 + 64 + 1 records in three batches (17 tiles, a full tile, one record).  The KEYSEL_ZERO corpus
mixes records made under the slot-0 keys of tables A, B, C of tests/key_tables.py, so each key
passes only its own third; the KEYSEL_IFID legs use that file's corpus.  Every expected bit comes
from the CPU checker (tests/orc.py); integer work, compared bit for bit.  GPU-side waits are the
test build's publish delay (3 ms) and a torch.cuda._sleep of under 5 ms."""
import ctypes
import functools

import numpy as np
import pytest

import key_tables as KT
import orc
import scion_hfv as hfv
import test_gpu_key_publish as KP
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = KP.DEV
CUTS = (0, 1029, 1093, 1094)
N = CUTS[-1]
PUBLISH_DELAY_US = 3000
SLEEP_CYCLES = 10_000_000        # torch.cuda._sleep: 20M cycles measured 8.3-9.6 ms (test_gpu_key_publish.py)


def key0(name):
    return KT.tables()[name][0][:16]


@functools.lru_cache(maxsize=None)
def zero_corpus():
    """(records u8[N, 64], {name: per batch the verdict words under table `name`'s slot-0 key})"""
    parts = []
    for i, name in enumerate(KT.NAMES):
        hk, _ = orc.key_table(key0(name))
        parts.append(orc.gen_records(N // 3 + 1, hk, 0, seed=orc.SEED_RECORDS + 16 + i))
    recs = np.concatenate(parts)[np.random.default_rng(2).permutation(3 * (N // 3 + 1))[:N]].copy()
    want = {}
    for name in KT.NAMES:
        hk, valid = orc.key_table(key0(name))
        w = orc.verify_records(recs, hk, valid, 0)
        p = np.unpackbits(w.view(np.uint8), bitorder="little")[:N].astype(bool)
        assert N // 4 < int(p.sum()) < N // 2, "a slot-0 key passes about its own third"
        want[name] = [KT.pack_bits(p[a:b]) for a, b in zip(CUTS[:-1], CUTS[1:])]
    return recs, want


def ifid_want(name):
    p = KT.want_bool()[name][:N]
    return [KT.pack_bits(p[a:b]) for a, b in zip(CUTS[:-1], CUTS[1:])]


class Batches:
    """Three batches over one device corpus, with fresh bitmaps pre-filled with ones."""

    def __init__(self, d):
        self.bits = [torch.full(((b - a + 63) // 64,), -1, dtype=torch.int64, device=DEV)
                     for a, b in zip(CUTS[:-1], CUTS[1:])]
        self.arr = hfv.Ctx.service_batches([(d.data_ptr() + 64 * a, b - a, t)
                                            for (a, b), t in zip(zip(CUTS[:-1], CUTS[1:]), self.bits)])

    def check(self, want, what):
        for k, (t, w) in enumerate(zip(self.bits, want)):
            assert np.array_equal(KP.host(t).view(np.uint64), w), "%s: batch %d" % (what, k)


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    torch.cuda.synchronize()
    c.synchronize()
    c.close()


def test_key_travels_by_value_across_streams(request, ctx):
    """(a) Slot 0 holds A's key; a verify on s1 sits behind the publish delay.  Slot 0 then gets
    B's key and a verify runs on s2.  s1's bitmap is A's truth, s2's is B's."""
    if rerun_on_test_build(request):   # hfv_debug_publish_delay: runs on lib/libscionhfv_test.so
        return
    recs, want = zero_corpus()
    d = KP.dev(recs)
    s1 = torch.cuda.Stream()
    s2 = KP.concurrent_with(s1)
    b1, b2, b3 = Batches(d), Batches(d), Batches(d)
    torch.cuda.synchronize()
    try:
        hfv.Ctx.debug_publish_delay(PUBLISH_DELAY_US)
        ctx.key_add(0, key0("A"))
        ctx.verify_batches(b1.arr, stream=s1)      # publishes on s1: spin, copy, then the kernel
        ctx.key_add(0, key0("B"))
        ctx.verify_batches(b2.arr, stream=s2)
        ctx.verify_batches(b3.arr, stream=s1)      # no publish: s1 again, now under B's key
    finally:
        hfv.Ctx.debug_publish_delay(0)
    torch.cuda.synchronize()
    b1.check(want["A"], "s1 under A")
    b2.check(want["B"], "s2 under B")
    b3.check(want["B"], "s1 under B")


def test_destroyed_stream_of_zero_key_launches_leaves_nothing(ctx):
    """(b) KEYSEL_ZERO verifies on a caller stream that is then destroyed (hipStreamDestroy); the ctx
    switches to KEYSEL_IFID and publishes three 256-key tables in turn from other streams."""
    L = hfv.lib()
    create, destroy, sync = L.hipStreamCreateWithFlags, L.hipStreamDestroy, L.hipStreamSynchronize
    create.argtypes, create.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], ctypes.c_int
    for f in (destroy, sync):
        f.argtypes, f.restype = [ctypes.c_void_p], ctypes.c_int
    recs, want = zero_corpus()
    dz, di = KP.dev(recs), KP.dev(KT.corpus()[0][:N])
    torch.cuda.synchronize()
    for name in "AB":
        ctx.key_add(0, key0(name))
        s = ctypes.c_void_p()
        assert create(ctypes.byref(s), 1) == 0 and s.value        # hipStreamNonBlocking
        b = Batches(dz)
        torch.cuda.synchronize()
        ctx.verify_batches(b.arr, stream=s.value)
        assert sync(s) == 0
        b.check(want[name], "KEYSEL_ZERO under %s" % name)
        assert destroy(s) == 0
    ctx.set_keysel(hfv.KEYSEL_IFID)
    for name in "ABC":
        KP.install(ctx, name)
        b = Batches(di)
        torch.cuda.synchronize()
        ctx.verify_batches(b.arr, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        b.check(ifid_want(name), "KEYSEL_IFID under %s" % name)


class Window(KP.Window):
    def open(self):
        torch.cuda.synchronize()
        self.t0.record(self.stream)
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(SLEEP_CYCLES)
        self.t1.record(self.stream)
        self.host0 = KP.time.perf_counter()


def test_reader_fence_holds_across_zero_key_launches(ctx):
    """(c) s1 verifies under table A with KEYSEL_IFID behind a sleep: it reads device table X.  On s2:
    KEYSEL_ZERO verifies, B installed, KEYSEL_ZERO verifies (publishing B into table Y), C
    installed, and a KEYSEL_IFID verify that publishes C into X -- which must wait for s1."""
    recs, want = zero_corpus()
    dz, di = KP.dev(recs), KP.dev(KT.corpus()[0][:N])
    s1 = torch.cuda.Stream()
    s2 = KP.concurrent_with(s1)
    warm, slow, last = Batches(di), Batches(di), Batches(di)
    z1, z2 = Batches(dz), Batches(dz)
    w = Window(s1)
    ctx.set_keysel(hfv.KEYSEL_IFID)
    KP.install(ctx, "A")
    ctx.verify_batches(warm.arr, stream=s2)        # warm-up: A is in table X
    w.open()
    ctx.verify_batches(slow.arr, stream=s1)
    w.mark()
    ctx.set_keysel(hfv.KEYSEL_ZERO)
    ctx.verify_batches(z1.arr, stream=s2)
    KP.install(ctx, "B")
    ctx.verify_batches(z2.arr, stream=s2)
    KP.install(ctx, "C")
    ctx.set_keysel(hfv.KEYSEL_IFID)
    ctx.verify_batches(last.arr, stream=s2)
    w.assert_open()
    w.report("reader fence across KEYSEL_ZERO launches")
    warm.check(ifid_want("A"), "warm-up under A")
    slow.check(ifid_want("A"), "s1 under A")
    z1.check(want["A"], "KEYSEL_ZERO under A")
    z2.check(want["B"], "KEYSEL_ZERO under B")
    last.check(ifid_want("C"), "s2 under C")
