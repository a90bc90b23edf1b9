"""hfv_verify_frames_batches on the GPU: a list of frame batches to verdict bits in as few launches
as the list allows (k_verify_frames_list).

The judge is independent of the code under test: hfv_frame_extract per frame on the host and the
record checker over the gathered fields, ANDed with status == 0, per batch (frames_list.expected).
Bit-equality with hfv_verify_frames_fused on the same batch is asserted beside it, never alone.

Every bitmap is pre-filled with 0xC3A5... and one guard word longer than needed; every status buffer
is pre-filled and three guard bytes longer; frames, lengths and ifindex arrays are compared
unchanged afterwards.  Integer work: every comparison is bit-exact.

The capped tests limit a launch to 1, 2 or 3 blocks with the test build's hfv_debug_batch_grid and
run in a child process on lib/libscionhfv_test.so (conftest.rerun_on_test_build).
tests/test_frames_list.py pins, on the CPU, where each list's batches fall against the block ranges.

`make fusededge` builds libraries 4-6 with one wrong step of the list kernel each
(csrc/hfv_frames_fused_kernel.hip); this module must fail on every one, by assertions alone: run it
with HFV_LIB=lib/libscionhfv_fusededgeN.so HFV_TEST_BUILD_CHILD=1."""
import ctypes
import errno

import numpy as np
import pytest

import frames_list as FL
import fused_deal as FD
import scion_hfv as hfv
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BITS_FILL = 0xC3A5C3A5C3A5C3A5     # neither 0 nor all-ones: a word never stored cannot pass for a verdict word
ST_FILL = 0x5A                     # no status value
ST_GUARD = 3
KEYSEL = pytest.mark.parametrize("keysel", [hfv.KEYSEL_ZERO, hfv.KEYSEL_IFID], ids=["zero", "ifid"])


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)                  # a fresh ctx: default keysel, no keys, empty set
    yield c
    c.synchronize()
    c.close()


@pytest.fixture()
def cap():
    """Sets the block cap of the launch; the default geometry is back afterwards."""
    yield hfv.Ctx.debug_batch_grid
    if hasattr(hfv.lib(), "hfv_debug_batch_grid"):   # (the parent process runs on the product library)
        hfv.Ctx.debug_batch_grid(0)


def setup(ctx, keysel, iset=FL.ISET):
    if keysel == hfv.KEYSEL_ZERO:
        ctx.key_add(0, FL.K1)
    else:
        ctx.key_add_batch(0, FL.ifid_raw())
    ctx.set_keysel(keysel)
    ctx.set_internal_ifindices(iset)


def fill_words(count):
    return torch.from_numpy(np.full(count, BITS_FILL, dtype=np.uint64).view(np.int64)).to(DEV)


SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
EMPTY_ARG = (None, 0, None, 0, None, None, None)             # an empty batch: NULL pointers


def to_dev(a):
    """A u8, u16 or u32 array as a device tensor of the same bytes."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED[a.dtype]).copy()).to(DEV)


class DevBatch:
    """One batch on the device: its inputs, its pre-filled outputs and the tuple the call takes."""

    def __init__(self, spec, share=None):
        """share: a DevBatch of the same frames, whose frame and length buffers this one takes."""
        self.spec, self.n = spec, spec.n
        if not spec.n:
            self.arg = EMPTY_ARG
            return
        b = FL.batch(spec)
        self.host = b
        n, slot = b.frames.shape
        if share is None:
            buf = torch.zeros(n * slot + 16, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            self.frames = buf[spec.shift:spec.shift + n * slot]
            self.frames.copy_(torch.from_numpy(b.frames.reshape(-1).copy()))
            self.lens = to_dev(b.lens)
        else:
            assert np.array_equal(share.host.frames, b.frames) and np.array_equal(share.host.lens, b.lens)
            self.frames, self.lens = share.frames, share.lens
        self.ifx = None if b.ifidx is None else to_dev(b.ifidx)
        self.words = FD.tiles_of(n)
        self.bits = fill_words(self.words + 1)
        self.status = torch.full((n + ST_GUARD,), ST_FILL, dtype=torch.uint8, device=DEV) if spec.status else None
        self.arg = (self.frames, slot, self.lens, n, self.bits, self.ifx, self.status)

    def refill(self):
        if self.n:
            self.bits.copy_(fill_words(self.words + 1))
            if self.status is not None:
                self.status.fill_(ST_FILL)

    def untouched(self):
        if not self.n:
            return True
        ok = (self.bits.cpu().numpy().view(np.uint64) == np.uint64(BITS_FILL)).all()
        return ok and (self.status is None or bool((self.status == ST_FILL).all()))

    def result(self, what):
        """(words, status or None) after a call; the guards and the inputs are checked here."""
        b = self.host
        assert np.array_equal(self.frames.cpu().numpy().reshape(b.frames.shape), b.frames), ("frames written", what)
        assert np.array_equal(self.lens.cpu().numpy().view(np.uint16), b.lens), ("lengths written", what)
        if self.ifx is not None:
            assert np.array_equal(self.ifx.cpu().numpy().view(np.uint32), b.ifidx), ("ifindex written", what)
        w = self.bits.cpu().numpy().view(np.uint64)
        assert w[self.words] == np.uint64(BITS_FILL), ("wrote past the bitmap", what)
        st = None
        if self.status is not None:
            st = self.status.cpu().numpy()
            assert (st[self.n:] == ST_FILL).all(), ("wrote status past n", what)
            st = st[:self.n]
        return w[:self.words], st


def upload(specs, share=()):
    """share: {position: earlier position whose frame and length buffers it takes}."""
    out = []
    for j, s in enumerate(specs):
        out.append(DevBatch(s, out[dict(share)[j]] if j in dict(share) else None))
    return out


def call(ctx, dbs, timed=False, stream=None):
    f = ctx.verify_frames_batches_timed if timed else ctx.verify_frames_batches
    return f([d.arg for d in dbs], stream=stream)


def compare(d, want, want_st, what):
    got, got_st = d.result(what)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, "%d bad words of %d, first %d: got %016x want %016x" % (
        len(bad), len(want), bad[0], int(got[bad[0]]), int(want[bad[0]])))
    if d.n % 64:
        assert int(got[-1]) >> (d.n % 64) == 0, ("a bit at or past n is set", what)
    if got_st is not None:
        assert np.array_equal(got_st, want_st), ("status", what)
    return got, got_st


def check_list(ctx, dbs, keysel, what, iset=FL.ISET, fused=False, **kw):
    """One list call against the oracle per batch (and beside it against verify_frames_fused on the
    same device buffers).  The ctx already holds the keys, the keysel and the set."""
    for d in dbs:
        d.refill()
    call(ctx, dbs)
    torch.cuda.synchronize()
    for j, d in enumerate(dbs):
        if not d.n:
            continue
        want, want_st = FL.expected(d.spec, keysel, iset, **kw)
        got, got_st = compare(d, want, want_st, (what, j, d.spec))
        if fused:
            d.refill()
            frames, slot, lens, n, bits, ifx, status = d.arg
            ctx.verify_frames_fused(frames, slot, lens, n, bits, ingress_ifindex=ifx, status=status)
            torch.cuda.synchronize()
            one, one_st = d.result((what, j, "fused"))
            assert np.array_equal(got, one), ("verify_frames_fused", what, j)
            assert got_st is None or np.array_equal(got_st, one_st), ("verify_frames_fused status", what, j)


# ---- the lists -----------------------------------------------------------------------------------

@KEYSEL
def test_ragged_list(ctx, keysel):
    """Batches of 1, 63, 64, 65, 37, 1025 and 4001 frames, each ending on a frame that passes:
    against the oracle and, beside it, against hfv_verify_frames_fused on the same batch."""
    setup(ctx, keysel)
    check_list(ctx, upload(FL.specs("ragged")), keysel, "ragged", fused=True)


@KEYSEL
def test_empty_batches(ctx, keysel):
    """Empty batches with NULL pointers at the head, in the middle and at the tail; count == 0 and a
    list of empty batches only launch nothing and return 0."""
    setup(ctx, keysel)
    check_list(ctx, upload(FL.specs("empties")), keysel, "empties")
    L = hfv.lib()
    assert L.hfv_verify_frames_batches(ctx._h, None, 0, None) == 0
    ctx.verify_frames_batches([])
    ctx.verify_frames_batches([EMPTY_ARG] * 3)
    assert ctx.verify_frames_batches_timed([]) == 0.0
    assert ctx.verify_frames_batches_timed([EMPTY_ARG] * 40) == 0.0
    torch.cuda.synchronize()


@KEYSEL
@pytest.mark.parametrize("name", ["split33", "split70"])
def test_split_lists(ctx, name, keysel):
    """33 and 70 non-empty batches of 1..130 frames: two and three launches."""
    setup(ctx, keysel)
    assert len(FL.launches(FL.specs(name))[0]) == {"split33": 2, "split70": 3}[name]
    check_list(ctx, upload(FL.specs(name)), keysel, name)


@KEYSEL
def test_mixed_staging(ctx, keysel):
    """Slots 2048, 256 and 144 (staged), 136 and 64 (direct) and a frame buffer 8 bytes past a
    16-byte boundary in one list, a launch per change; the window-edge corpus staged and direct."""
    setup(ctx, keysel)
    dbs = upload(FL.specs("mixed"))
    for d in dbs:
        assert (d.frames.data_ptr() % 16 == 0) == (d.spec.shift == 0)
    check_list(ctx, dbs, keysel, "mixed", fused=True)


@KEYSEL
def test_direction(ctx, keysel):
    """The set {5, 7}: batches with an ifindex array and with NULL, with and without status, the same
    frames twice with different ifindex arrays.  With an empty set every batch is external."""
    setup(ctx, keysel)
    dbs = upload(FL.specs("direction"), share={1: 0, 4: 0})  # one frame buffer in three batches
    assert dbs[0].frames.data_ptr() == dbs[1].frames.data_ptr() == dbs[4].frames.data_ptr()
    check_list(ctx, dbs, keysel, "direction", fused=True)
    ctx.set_internal_ifindices([])
    check_list(ctx, dbs, keysel, "direction, empty set", iset=())


@KEYSEL
def test_direction_capped(request, ctx, cap, keysel):
    """The same list on 1 and 2 blocks, where a wave passes from a batch without an ifindex array
    into one with it and back (tests/test_frames_list.py: PLACEMENT)."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    setup(ctx, keysel)
    dbs = upload(FL.specs("direction"))
    for blocks in (1, 2):
        cap(blocks)
        check_list(ctx, dbs, keysel, "direction, cap %d" % blocks)


# ---- keys ----------------------------------------------------------------------------------------

def test_keysel_zero_without_key_fails_closed(ctx):
    """Slot 0 added, then removed: no bit of any batch set, the status still exact."""
    ctx.key_add(0, FL.K1)
    ctx.key_remove(0)
    ctx.set_internal_ifindices(FL.ISET)
    dbs = upload(FL.specs("ragged"))
    check_list(ctx, dbs, hfv.KEYSEL_ZERO, "no key", nokey=True)
    for d in dbs:
        got, st = d.result("no key")
        assert not got.any() and (d.n < 256 or (st == 0).sum() > d.n // 2)


def test_keysel_ifid_partial_table(ctx):
    """The frames' slots (the AS interfaces 1..6) missing from the table: those bits are 0."""
    setup(ctx, hfv.KEYSEL_IFID)
    for k in range(1, 7):
        ctx.key_remove(k)
    dbs = upload(FL.specs("ragged"))
    check_list(ctx, dbs, hfv.KEYSEL_IFID, "partial table", partial=True)
    assert sum(int(FL.passes_of(FL.expected(d.spec, 1)[0], d.n).sum()) for d in dbs) > 500
    assert not any(d.result("partial")[0].any() for d in dbs)


# ---- tile dealing --------------------------------------------------------------------------------

class DealList:
    """A dealing list on the device: the batches' frames gathered from the cycled batch into one
    buffer, batch after batch, each batch with its own bitmap and status buffer."""

    def __init__(self, keysel, sizes):
        frames, lens, self.passes = FL.deal_case(keysel)
        self.sizes = sizes
        total = sum(sizes)
        i = torch.arange(total, device=DEV) % FL.CYCLE
        self.frames = torch.from_numpy(frames).to(DEV)[i].contiguous()
        self.lens = to_dev(lens)[i].contiguous()
        self.starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        self.bits = [fill_words(FD.tiles_of(n) + 1) for n in sizes]
        self.status = [torch.full((n + ST_GUARD,), ST_FILL, dtype=torch.uint8, device=DEV) for n in sizes]
        self.args = [(self.frames[s:s + n], FL.DEAL_SLOT, self.lens[s:s + n], n, b, None, st)
                     for s, n, b, st in zip(self.starts, sizes, self.bits, self.status)]

    def check(self, what):
        for j, (s, n, b, st) in enumerate(zip(self.starts, self.sizes, self.bits, self.status)):
            words = FD.tiles_of(n)
            want = FL.deal_words(self.passes, int(s), n)
            got = b.cpu().numpy().view(np.uint64)
            assert got[words] == np.uint64(BITS_FILL), ("wrote past the bitmap", what, j)
            bad = np.nonzero(got[:words] != want)[0]
            assert not len(bad), (what, "batch %d of %d frames: %d bad words of %d, first %d: got %016x want %016x" % (
                j, n, len(bad), words, bad[0], int(got[bad[0]]), int(want[bad[0]])))
            assert (st[n:] == ST_FILL).all() and not (st[:n] == ST_FILL).any(), ("status", what, j)


def run_deal(ctx, keysel, kind, blocks, what):
    dl = DealList(keysel, FL.deal_sizes(kind, keysel, blocks))
    ctx.verify_frames_batches(dl.args)
    torch.cuda.synchronize()
    dl.check(what)


@KEYSEL
def test_tile_dealing_capped(request, ctx, cap, keysel):
    """1, 2 and 3 blocks: every wave claims three tiles or more over many small batches and over a
    few large ones, block ranges start inside batches and a wave's forward step passes several
    batches (tests/test_frames_list.py: DEAL_PLACEMENT)."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    setup(ctx, keysel, iset=())
    for blocks in FD.CAPS:
        cap(blocks)
        for kind in ("small", "large"):
            run_deal(ctx, keysel, kind, blocks, (keysel, kind, "cap %d" % blocks))


@KEYSEL
@pytest.mark.parametrize("kind", ["small", "large"])
def test_tile_dealing_real_grid(ctx, kind, keysel):
    """The uncapped grid: 128 small batches in four launches, and five large ones on one block per
    CU with three tiles per wave and one over."""
    setup(ctx, keysel, iset=())
    run_deal(ctx, keysel, kind, FD.REAL_GRID, (keysel, kind, "real grid"))


@KEYSEL
def test_lists_capped(request, ctx, cap, keysel):
    """The ragged, split and mixed lists on 1, 2 and 3 blocks."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    setup(ctx, keysel)
    for name in ("ragged", "split70", "mixed"):
        dbs = upload(FL.specs(name))
        for blocks in FD.CAPS:
            cap(blocks)
            check_list(ctx, dbs, keysel, "%s, cap %d" % (name, blocks))


# ---- stream order, key publication -------------------------------------------------------------

def test_stream_ordered(ctx):
    """H2D copies of every batch's frames, lengths and ifindices behind a few ms of other work, the
    list call and a torch consumer of the bitmaps on one non-default stream, one synchronize at the
    end."""
    setup(ctx, hfv.KEYSEL_ZERO)
    specs = FL.specs("direction")
    hosts = [FL.batch(s) for s in specs]
    pinned = [(torch.from_numpy(b.frames.copy()).pin_memory(),
               torch.from_numpy(b.lens.view(np.int16).copy()).pin_memory(),
               None if b.ifidx is None else torch.from_numpy(b.ifidx.view(np.int32).copy()).pin_memory())
              for b in hosts]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = [tuple(None if x is None else torch.zeros(x.shape, dtype=x.dtype, device=DEV) for x in p) for p in pinned]
        bits = [torch.full((FD.tiles_of(sp.n),), -1, dtype=torch.int64, device=DEV) for sp in specs]
        torch.cuda._sleep(5_000_000)                         # the producer runs late
        for (df, dl, di), (f, ln, i) in zip(dev, pinned):
            df.copy_(f, non_blocking=True)
            dl.copy_(ln, non_blocking=True)
            if i is not None:
                di.copy_(i, non_blocking=True)
        ctx.verify_frames_batches([(df, sp.slot, dl, sp.n, b, di) for (df, dl, di), sp, b in zip(dev, specs, bits)],
                                  stream=s)
        outs = [b.clone() for b in bits]                     # the consumer
    s.synchronize()
    for sp, o in zip(specs, outs):
        assert np.array_equal(o.cpu().numpy().view(np.uint64), FL.expected(sp, 0)[0]), sp


@KEYSEL
def test_key_publication(ctx, keysel):
    """Two list calls on one stream held behind a sleep, a key change between them: each call's
    bitmaps are those of the keys it was enqueued with (the pattern of test_gpu_frames_fused.py's
    test_key_publication).  A third set of bitmaps holds the warm-up call's verdicts."""
    from test_gpu_key_publish import Window
    other = bytes(range(16))
    setup(ctx, keysel)
    specs = FL.specs("split33")
    dbs = [upload(specs) for _ in range(3)]
    s = torch.cuda.Stream()
    call(ctx, dbs[2], stream=s)                              # warm-up: the first table is published
    w = Window(s)
    w.open()
    call(ctx, dbs[0], stream=s)
    w.mark()
    for ifid in range(0 if keysel == hfv.KEYSEL_ZERO else 1, 7):
        ctx.key_add(ifid, other)
    call(ctx, dbs[1], stream=s)
    w.assert_open()
    w.report("frame list key publication")
    raw2 = bytearray(FL.keys(keysel)[0])
    for ifid in range(0 if keysel == hfv.KEYSEL_ZERO else 1, 7):
        raw2[16 * ifid:16 * ifid + 16] = other
    npass = npass2 = 0
    for j, sp in enumerate(specs):
        want, want_st = FL.expected(sp, keysel)
        want2, _ = FL.expected(sp, keysel, raw=bytes(raw2))
        npass, npass2 = npass + int(FL.passes_of(want, sp.n).sum()), npass2 + int(FL.passes_of(want2, sp.n).sum())
        compare(dbs[0][j], want, want_st, ("first call", j))
        compare(dbs[2][j], want, want_st, ("warm-up call", j))
        compare(dbs[1][j], want2, want_st, ("second call", j))
    assert npass > 500 and npass2 == 0


# ---- arguments, timed form -----------------------------------------------------------------------

def test_arguments(ctx):
    """Each check fails on batch 0 and on a later batch, the error text names the batch, and every
    bitmap and status buffer is still at its fill."""
    setup(ctx, hfv.KEYSEL_ZERO)
    dbs = upload(FL.specs("empties")[1:])                    # batches 0, 3 and 4 are live, the others empty
    live = [j for j, d in enumerate(dbs) if d.n]
    assert live == [0, 3, 4]
    L, h = hfv.lib(), ctx._h
    E = -errno.EINVAL
    ms = ctypes.c_float(-1.0)
    good = [d.arg for d in dbs]

    def bad(j, **change):
        """The list with batch j's tuple changed; both forms must fail alike, naming batch j."""
        fields = dict(zip(("frames", "slot", "lens", "n", "pass_bits", "ifx", "status"), good[j]))
        fields.update(change)
        args = list(good)
        args[j] = tuple(fields[k] for k in ("frames", "slot", "lens", "n", "pass_bits", "ifx", "status"))
        arr = hfv.Ctx.frame_batches(args)
        for rc in (L.hfv_verify_frames_batches(h, arr, len(args), None),
                   L.hfv_verify_frames_batches_timed(h, arr, len(args), None, ctypes.byref(ms))):
            assert rc == E, (j, change)
            assert L.hfv_last_error().decode().startswith("batch %d: " % j), (j, change, L.hfv_last_error())

    for j in (live[0], live[-1]):
        slot, bits = good[j][1], good[j][4].data_ptr()
        bad(j, slot=slot + 4)                                # slot % 8
        bad(j, slot=56)                                      # slot < 64
        bad(j, slot=(1 << 24) + 8)                           # slot > 16 MiB
        bad(j, n=(1 << 36) + 1)                              # n > 2^36
        bad(j, frames=None)
        bad(j, lens=None)
        bad(j, pass_bits=None)
        bad(j, pass_bits=bits + 4)                           # bitmap not 8-byte aligned
    arr = hfv.Ctx.frame_batches(good)
    assert L.hfv_verify_frames_batches(None, arr, len(good), None) == E
    assert L.hfv_verify_frames_batches(h, None, len(good), None) == E
    assert L.hfv_verify_frames_batches_timed(h, arr, len(good), None, None) == E
    torch.cuda.synchronize()
    assert all(d.untouched() for d in dbs), "a rejected call wrote an output"
    # and the good list still runs
    check_list(ctx, dbs, hfv.KEYSEL_ZERO, "after the rejected calls")


@KEYSEL
def test_timed_form(ctx, keysel):
    """A positive time and the same bits, over three launches."""
    setup(ctx, keysel)
    dbs = upload(FL.specs("split70"))
    ms = call(ctx, dbs, timed=True)
    assert 0.0 < ms < 100.0
    for j, d in enumerate(dbs):
        compare(d, *FL.expected(d.spec, keysel), ("timed", j))
