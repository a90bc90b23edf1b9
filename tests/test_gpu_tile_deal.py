"""The tile dealing of k_verify_batches -- block ranges, the static first tile and the claimed ones,
batch_map over cum[], the prefetch across a batch boundary and its clamp past the block's range,
the 64-word verdict stash with a bitmap address per lane, the fail-closed loop -- on the lists of
tests/tile_deal.py, against the CPU checker's verdicts of the base records (judged once, on the
host; nothing expected here comes from the library).  Integer work: every comparison is bit-exact.

Where a wave must verify many tiles the launch is capped at 1, 2 or 3 blocks with the test
build's hfv_debug_batch_grid, so those tests run in a child process on lib/libscionhfv_test.so
(conftest.rerun_on_test_build); a list of 2048 tiles then gives a wave 40 to 128 tiles over as
many as 42 batches.  The real-grid tests need no hook.  The lists are built for the block count
they run on (tests/test_tile_deal.py pins where their batches fall for 1, 2, 3 and 256 blocks).

Every batch's bitmap lies between two guard words on either side and is pre-filled with ones.
For every batch: the words equal the checker's, the guards are intact, no bit at or past n is
set, and an empty batch's word is untouched.

A mutant build (make tiledeal) already has the hook: run it with
HFV_LIB=lib/libscionhfv_tiledealN.so HFV_TEST_BUILD_CHILD=1, which runs every test body in place.

Out of scope: the resident service's own dealing (k_verify_service; tests/test_gpu_svc_deal.py),
and the split of a launch at 2^31 tiles, which no test size reaches."""
import numpy as np
import pytest

import hf_bits as HB
import scion_hfv as hfv
import tile_deal as TD
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
FILL = 0xFFFFFFFFFFFFFFFF
CAPS = (1, 2, 3)
KEYSELS = (0, 1)
LAYOUTS = tuple(TD.LAYOUTS)
lid = ["%d-%d" % l for l in LAYOUTS]

_DEV = {}


def dev_base(keysel):
    """The base records on the device, uploaded once."""
    if keysel not in _DEV:
        _DEV[keysel] = torch.from_numpy(np.array(TD.base(keysel)[0])).to(DEV)
    return _DEV[keysel]


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()


@pytest.fixture()
def cap():
    """Sets the block cap of the batch-list launch; the default geometry is back afterwards."""
    yield hfv.Ctx.debug_batch_grid
    if hasattr(hfv.lib(), "hfv_debug_batch_grid"):   # (the parent process runs on the product library)
        hfv.Ctx.debug_batch_grid(0)


def setup(ctx, keysel, layout, slots=None):
    raw = TD.keys(1)[0]
    for k in (range(256) if keysel else range(1)) if slots is None else slots:
        ctx.key_add(k, raw[16 * k:16 * k + 16])
    ctx.set_keysel(keysel)
    ctx.set_record_layout(*layout)


class Arena:
    """One device tensor with every batch's bitmap: guard, guard, words (ones), guard, guard."""

    def __init__(self, sz):
        self.sz = sz
        self.at, p = [], 0
        for n in sz:
            self.at.append(p + 2)
            p += max(1, (n + 63) // 64) + 4
        host = np.full(p, GUARD, dtype=np.uint64)
        for a, n in zip(self.at, sz):
            host[a:a + max(1, (n + 63) // 64)] = FILL
        self.t = torch.from_numpy(host.view(np.int64)).to(DEV)

    def bits(self, j):
        return self.t[self.at[j]:]

    def check(self, want, what):
        """want: per batch the expected words (None: an empty batch)."""
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().view(np.uint64)
        for j, (a, n, w) in enumerate(zip(self.at, self.sz, want)):
            nw = max(1, (n + 63) // 64)
            where = (what, "batch %d of %d" % (j, len(self.sz)), "n=%d" % n)
            assert (got[a - 2:a] == GUARD).all() and (got[a + nw:a + nw + 2] == GUARD).all(), ("guard written", where)
            if n == 0:
                assert got[a] == FILL, ("an empty batch was written to", where)
                continue
            words = got[a:a + nw]
            if n % 64:
                assert int(words[-1]) >> (n % 64) == 0, ("a bit at or past n is set", where)
            bad = np.nonzero(words != w)[0]
            assert not len(bad), (where, "%d bad words, first %d: got %016x want %016x" % (
                len(bad), bad[0], int(words[bad[0]]), int(w[bad[0]])))


class DevList:
    """A list of tests/tile_deal.py on the device: every batch gathered from the uploaded base
    into its own stride and layout, and the arena of bitmaps."""

    def __init__(self, name, B, keysel, layout):
        self.name, self.sz = name, TD.sizes(name, B)
        base, s = dev_base(keysel), TD.start(name)
        self.recs, off = [], 0
        for n, stride in zip(self.sz, TD.strides(self.sz, layout)):
            r = torch.full((max(n, 1), stride), TD.FILLER, dtype=torch.uint8, device=DEV)
            if n:
                i = (torch.arange(n, device=DEV) + (s + off)) % TD.K
                r[:, layout[0]:layout[0] + 8] = base[i, 40:48]
                r[:, layout[1]:layout[1] + 12] = base[i, 48:60]
            self.recs.append((r, stride))
            off += n
        self.arena = Arena(self.sz)

    def batches(self):
        return [(r, n, self.arena.bits(j), stride) for j, (n, (r, stride)) in enumerate(zip(self.sz, self.recs))]

    def check(self, passes, what):
        self.arena.check(TD.expected(self.name, self.sz, passes), what)


def run_list(ctx, name, B, keysel, layout, passes, what, timed=False):
    L = DevList(name, B, keysel, layout)
    if timed:
        assert ctx.verify_batches_timed(L.batches()) > 0
    else:
        ctx.verify_batches(L.batches())
    L.check(passes, (name, "B=%d" % B) + tuple(what))


@pytest.mark.parametrize("layout", LAYOUTS, ids=lid)
@pytest.mark.parametrize("keysel", KEYSELS)
def test_capped_lists(request, ctx, cap, keysel, layout):
    """Every list under 1, 2 and 3 blocks."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    setup(ctx, keysel, layout)
    passes = TD.base(keysel)[1]
    for B in CAPS:
        cap(B)
        for name in TD.NAMES:
            run_list(ctx, name, B, keysel, layout, passes, (keysel, layout))


@pytest.mark.parametrize("layout", LAYOUTS, ids=lid)
@pytest.mark.parametrize("keysel", KEYSELS)
def test_real_grid_lists(ctx, keysel, layout):
    """train, edges and the three just-over shapes on one block per CU: about 20 tiles per block
    and 7 over, the lists built for the CU count the ctx reads."""
    B = torch.cuda.get_device_properties(0).multi_processor_count
    setup(ctx, keysel, layout)
    passes = TD.base(keysel)[1]
    for name in ("train", "edges", "just16", "just1", "just2"):
        TD.assert_no_word_can_stand_in(name, TD.sizes(name, B), passes)   # (test_tile_deal.py: for 256 CUs)
        run_list(ctx, name, B, keysel, layout, passes, (keysel, layout))


@pytest.mark.parametrize("layout", LAYOUTS, ids=lid)
def test_capped_partial_key_table(request, ctx, cap, layout):
    """KEYSEL_IFID with only the even slots installed: the records of empty slots fail closed in
    the middle of waves that verify many tiles."""
    if rerun_on_test_build(request):
        return
    setup(ctx, 1, layout, slots=range(0, 256, 2))
    passes = TD.judge(TD.base(1)[0], 1, valid=HB.partial_valid())
    for B in (1, 3):
        cap(B)
        for name in ("train", "edges", "over64"):
            run_list(ctx, name, B, 1, layout, passes, ("even slots", layout))


@pytest.mark.parametrize("layout", LAYOUTS, ids=lid)
def test_capped_no_key_in_slot_0(request, ctx, cap, layout):
    """KEYSEL_ZERO with slot 0 empty (slots 1..255 installed): the fail-closed loop over block
    ranges of many batches.  Every word of every batch is 0 and nothing else is written."""
    if rerun_on_test_build(request):
        return
    setup(ctx, 0, layout, slots=range(1, 256))
    for B in (1, 3):
        cap(B)
        for name in ("train", "over64"):
            run_list(ctx, name, B, 0, layout, np.zeros(TD.K, dtype=bool), ("no key", layout))


def test_capped_timed(request, ctx, cap):
    """hfv_verify_batches_timed on train under 2 blocks: the same verdicts, and a time."""
    if rerun_on_test_build(request):
        return
    setup(ctx, 0, LAYOUTS[0])
    cap(2)
    run_list(ctx, "train", 2, 0, LAYOUTS[0], TD.base(0)[1], ("timed",), timed=True)


@pytest.mark.parametrize("keysel", KEYSELS)
def test_capped_single_through_verify_records(request, ctx, cap, keysel):
    """hfv_verify_records is the batch-list kernel with one batch: 2048 tiles on 1 and 3 blocks."""
    if rerun_on_test_build(request):
        return
    passes = TD.base(keysel)[1]
    for layout in LAYOUTS:
        setup(ctx, keysel, layout)
        for B in (1, 3):
            cap(B)
            L = DevList("single", B, keysel, layout)
            (r, n, bits, stride), = L.batches()
            ctx.verify_records(r, n, bits, stride=stride)
            L.check(passes, ("verify_records", "B=%d" % B, keysel, layout))


def test_capped_single_through_verify_frames(request, ctx, cap):
    """hfv_verify_frames' verify step on one block: the base records inside minimal valid frames.
    Every frame has status 0 and the bits equal the record checker's."""
    if rerun_on_test_build(request):
        return
    keysel = 0
    setup(ctx, keysel, (0, 8))
    recs, passes = TD.base(keysel)
    fr, length = TD.frames(recs)
    n, = TD.sizes("single", 1)
    i = (torch.arange(n, device=DEV) + TD.start("single")) % TD.K
    frames = torch.from_numpy(fr).to(DEV)[i].contiguous()
    lens = torch.full((n,), length, dtype=torch.int16, device=DEV)
    out = torch.full((n, hfv.FRAME_REC_STRIDE), TD.FILLER, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    arena = Arena([n])
    cap(1)
    ctx.verify_frames(frames, fr.shape[1], lens, n, out, status, arena.bits(0))
    torch.cuda.synchronize()
    assert not status.any().item(), "a frame did not parse"
    arena.check(TD.expected("single", [n], passes), ("verify_frames",))
