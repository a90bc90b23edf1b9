"""The tile dealing of k_verify_service -- weighted block shares of every batch, the block-local tile
counter that runs on across batches, the LDS descriptor cache and its forward search, the batches
taken from the kernel arguments, the relay's read-ahead with the stop inside it, the 64-word
verdict stash with its deferred completion counts -- on the lists of tests/svc_deal.py, against the
CPU checker's verdicts of tests/tile_deal.py's base records (judged once, on the host; nothing
expected here comes from the library).  Integer work: every comparison is bit-exact.

Small grids come from the public hfv_service_set_grid, so all but the weighted leg run on the
product library; one block then verifies a whole list with 15 waves.  The lists are built for the
block count they run on (tests/test_svc_deal.py pins where they fall for 1, 2, 3 and 256 blocks).

Every batch's bitmap lies between two guard words on either side and is pre-filled with ones.
For every batch: the words equal the checker's, the guards are intact, no bit at or past n is
set, and an empty batch's word is untouched.  After every grid its block count and the relay's
inline and relayed counters equal the model's.  Every wait has a 20 s timeout.

The matrix (tests/svc_deal.py MATRIX; list[:run length]/entry point/keysel/layout of
tile_deal.LAYOUTS; G=0: one block per CU).  Entry points: run = hfv_service_run, async =
hfv_service_run_async and a device synchronize, live = hfv_service_submitv in bursts of 7 on a
running grid, stopped = hfv_service_submitv of the whole list on a stopped service.  The strides
cycle per batch.  Every list and every entry point meets every grid (tests/test_svc_deal.py):

    G=1  fill/run/k0/l0  train/async/k1/l1  edges/live/k0/l1  counts:127/stopped/k1/l0  over_ring/run/k1/l1  fewer/async/k0/l0
    G=2  fill/async/k1/l1  train/live/k0/l0  edges/stopped/k1/l0  counts:64/run/k0/l1  over_ring/async/k0/l0  fewer/live/k1/l1
    G=3  fill/live/k0/l1  train/stopped/k1/l0  edges/run/k1/l1  counts:128/async/k0/l0  over_ring/live/k1/l0  fewer/stopped/k0/l1
    G=0  fill/stopped/k1/l0  train/run/k0/l1  edges/async/k0/l0  counts:65/live/k1/l1  over_ring/stopped/k0/l1  fewer/run/k1/l0

Beside it: counts at each of its six run lengths through run and async on 1 block and the real
grid; a partial key table and an empty slot 0 on 1 block; set_grid between grids of one ctx; and,
in a child process on the test build (hfv_debug_service_set_weights), unequal weights.

A mutant build (make svcdeal) has the hook: run it with HFV_LIB=lib/libscionhfv_svcdealN.so
HFV_TEST_BUILD_CHILD=1, which runs every test body in place."""
import errno

import numpy as np
import pytest

import hf_bits as HB
import scion_hfv as hfv
import svc_deal as SD
import tile_deal as TD
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
FILL = 0xFFFFFFFFFFFFFFFF
WAIT_MS = 20000
LAYOUTS = tuple(TD.LAYOUTS)

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
    c.service_stop()
    c.close()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def setup(ctx, keysel, layout, slots=None):
    raw = TD.keys(1)[0]
    for k in (range(256) if keysel else range(1)) if slots is None else slots:
        ctx.key_add(k, raw[16 * k:16 * k + 16])
    ctx.set_keysel(keysel)
    ctx.set_record_layout(*layout)


class DevList:
    """A list on the device: every batch gathered from the uploaded base into its own stride and
    layout, and one tensor with every batch's bitmap: guard, guard, words (ones), guard, guard."""

    def __init__(self, tag, sz, keysel, layout):
        self.tag, self.sz = tag, sz
        base, s = dev_base(keysel), TD.start(tag)
        self.recs, off = [], 0
        for n, stride in zip(sz, TD.strides(sz, layout)):
            r = torch.full((max(n, 1), stride), TD.FILLER, dtype=torch.uint8, device=DEV)
            if n:
                i = (torch.arange(n, device=DEV) + (s + off)) % TD.K
                r[:, layout[0]:layout[0] + 8] = base[i, 40:48]
                r[:, layout[1]:layout[1] + 12] = base[i, 48:60]
            self.recs.append((r, stride))
            off += n
        self.at, p = [], 0
        for n in sz:
            self.at.append(p + 2)
            p += max(1, SD.tiles(n)) + 4
        host = np.full(p, GUARD, dtype=np.uint64)
        for a, n in zip(self.at, sz):
            host[a:a + max(1, SD.tiles(n))] = FILL
        self.t = torch.from_numpy(host.view(np.int64)).to(DEV)
        torch.cuda.synchronize()                       # a post is host-ordered: records and bitmaps are complete

    def batches(self):
        return [(r, n, self.t[a:], stride) for n, a, (r, stride) in zip(self.sz, self.at, self.recs)]

    def check(self, passes, what):
        torch.cuda.synchronize()
        got = self.t.cpu().numpy().view(np.uint64)
        for j, (a, n, w) in enumerate(zip(self.at, self.sz, TD.expected(self.tag, self.sz, passes))):
            nw = max(1, SD.tiles(n))
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


def wait(ctx, t):
    """hfv_service_wait with the finite timeout.  A ticket that does not complete means the grid
    hangs: the session ends there, so that nothing more is started on that GPU."""
    try:
        ctx.service_wait(t, WAIT_MS)
    except hfv.HfvError as e:
        if e.code == -errno.ETIMEDOUT:
            pytest.exit("ticket %d not complete after %d ms" % (t, WAIT_MS), returncode=3)
        raise


def post(ctx, batches, entry):
    """The batches through one entry point, to the grid's end; returns the tickets, all complete."""
    if entry == "run":
        ts, ms = ctx.service_run(batches)
        assert ms >= 0 and not ctx.service_running
    elif entry == "async":
        ts = ctx.service_run_async(batches)
        torch.cuda.synchronize()
    else:
        if entry == "live":
            ctx.service_start()
            assert ctx.service_running
            ts = []
            for i in range(0, len(batches), 7):
                ts += ctx.service_submitv(batches[i:i + 7])
        else:
            assert not ctx.service_running
            ts = ctx.service_submitv(batches)
        for t in ts:
            wait(ctx, t)
    assert len(ts) == len(batches) and ts == list(range(ts[0], ts[0] + len(ts)))
    for t in ts:
        assert ctx.service_poll(t), ("ticket not complete", t)
    ctx.service_stop()
    return ts


def check_grid(ctx, count, entry, G, what):
    """The grid that just ended: its blocks, and the relay's counters against the model."""
    assert ctx.service_grid() == G, (what, ctx.service_grid())
    rel, p = ctx.service_relay(), SD.posting(count, entry)
    print(what, entry, "G=%d" % G, rel)
    assert (rel["inline"], rel["relayed"]) == (p.inline, p.relayed), (what, rel, p)
    if p.up_front:                                     # nothing was posted after the launch
        assert rel["block_waits"] == 0, (what, rel)


def run_list(ctx, name, G, entry, keysel, layout, passes, L=None, sz=None, what=()):
    """One list on the grid the ctx is set to (G blocks), through one entry point."""
    sz = SD.sizes(name, G, L) if sz is None else sz
    what = (name, L, "G=%d" % G, entry, keysel, layout) + tuple(what)
    dl = DevList(SD.tag(name, L), sz, keysel, layout)
    ts = post(ctx, dl.batches(), entry)
    dl.check(passes, what)
    check_grid(ctx, len(sz), entry, G, what)
    return ts


@pytest.mark.parametrize("name,grid,entry,keysel,ly,L", SD.MATRIX,
                         ids=["%s%s-G%d-%s-k%d-l%d" % (m[0], m[5] or "", m[1], m[2], m[3], m[4]) for m in SD.MATRIX])
def test_matrix(ctx, name, grid, entry, keysel, ly, L):
    """The written-down matrix: every list and every entry point on 1, 2, 3 blocks and the real grid."""
    G = grid or cus()
    setup(ctx, keysel, LAYOUTS[ly])
    ctx.service_set_grid(grid)
    passes = TD.base(keysel)[1]
    if not grid:                                       # (test_svc_deal.py: for 256 CUs)
        TD.assert_no_word_can_stand_in(SD.tag(name, L), SD.sizes(name, G, L), passes)
    run_list(ctx, name, G, entry, keysel, LAYOUTS[ly], passes, L)


@pytest.mark.parametrize("entry", ["run", "async"])
@pytest.mark.parametrize("grid", [1, 0])
def test_run_lengths(ctx, grid, entry):
    """counts at 63, 64, 65, 127, 128 and 129 batches: the stop as inl[63], as the first relayed
    descriptor, in ring slot 127, and behind a ring filled before the launch."""
    G = grid or cus()
    keysel, layout = (0, LAYOUTS[0]) if entry == "run" else (1, LAYOUTS[1])
    setup(ctx, keysel, layout)
    ctx.service_set_grid(grid)
    for L in SD.RUN_LENGTHS:
        run_list(ctx, "counts", G, entry, keysel, layout, TD.base(keysel)[1], L)


@pytest.mark.parametrize("name", ["fill", "train"])
def test_partial_key_table(ctx, name):
    """KEYSEL_IFID with only the even slots installed, on one block: the records of empty slots
    fail closed in the middle of waves that verify many tiles."""
    setup(ctx, 1, LAYOUTS[0], slots=range(0, 256, 2))
    ctx.service_set_grid(1)
    passes = TD.judge(TD.base(1)[0], 1, valid=HB.partial_valid())
    run_list(ctx, name, 1, "run", 1, LAYOUTS[0], passes, what=("even slots",))


@pytest.mark.parametrize("name", ["fill", "train"])
def test_no_key_in_slot_0(ctx, name):
    """KEYSEL_ZERO with slot 0 empty (slots 1..255 installed), on one block: every word of every
    batch is 0, not the pre-fill, and nothing else is written."""
    setup(ctx, 0, LAYOUTS[1], slots=range(1, 256))
    ctx.service_set_grid(1)
    run_list(ctx, name, 1, "async", 0, LAYOUTS[1], np.zeros(TD.K, dtype=bool), what=("no key",))


def test_set_grid_between_grids(ctx):
    """hfv_service_set_grid at a batch boundary of one ctx: 1 block, then 3 (set while the first
    grid still runs: it is stopped at the boundary), then one per CU.  Tickets stay monotonic and
    every grid's bitmaps are right."""
    keysel, layout = 0, LAYOUTS[0]
    setup(ctx, keysel, layout)
    passes = TD.base(keysel)[1]
    ctx.service_set_grid(1)
    a = DevList(SD.tag("edges"), SD.edges(1), keysel, layout)
    b = DevList(SD.tag("fewer"), SD.fewer(3), keysel, layout)
    c = DevList(SD.tag("train"), SD.train(cus()), keysel, layout)
    ta = ctx.service_submitv(a.batches())
    for t in ta:
        wait(ctx, t)
    assert ctx.service_running
    ctx.service_set_grid(3)
    assert not ctx.service_running and ctx.service_grid() == 1
    tb = ctx.service_submitv(b.batches())
    for t in tb:
        wait(ctx, t)
    ctx.service_set_grid(0)
    assert not ctx.service_running and ctx.service_grid() == 3
    tc, _ = ctx.service_run(c.batches())
    assert ctx.service_grid() == cus()
    ts = ta + tb + tc
    assert ts == list(range(ts[0], ts[0] + len(ts))) and all(ctx.service_poll(t) for t in ts)
    a.check(passes, ("set_grid", 1))
    b.check(passes, ("set_grid", 3))
    c.check(passes, ("set_grid", 0))


@pytest.mark.parametrize("w0", [512, 2048])
def test_weighted_shares(request, ctx, w0):
    """Unequal block weights (svc_deal.PATTERN, block 0 at either end of the clamp), set before every
    grid because svc_balance may move them after one: a train-shaped list of 20 G + 7 tiles on 3,
    8, 9, 17 blocks and the real grid, and fill on 3 blocks.  Every tile is verified exactly where
    it belongs, and the grid was launched with the weights that were set."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    w = list(SD.PATTERN) + [w0]
    assert ctx.service_weights() == [SD.UNIT] * 9
    with pytest.raises(hfv.HfvError):
        ctx.debug_service_set_weights([511] + w[1:])
    with pytest.raises(hfv.HfvError):
        ctx.debug_service_set_weights(w[:8] + [2049])
    assert ctx.service_weights() == [SD.UNIT] * 9
    keysel, layout = (0, LAYOUTS[1]) if w0 == 512 else (1, LAYOUTS[0])
    setup(ctx, keysel, layout)
    passes = TD.base(keysel)[1]
    for grid, name in ((3, "train"), (8, "train"), (9, "train"), (17, "train"), (0, "train"), (3, "fill")):
        G = grid or cus()
        sz = SD.weighted_train(G) if name == "train" else SD.fill(G)
        TD.assert_no_word_can_stand_in(SD.tag(name), sz, passes)
        sh = SD.shares(SD.weighted_T(G), G, SD.PATTERN, w0)
        assert all(x < y for x, y in sh) and not any(x == y for x, y in zip(sh, SD.shares(SD.weighted_T(G), G)))
        ctx.service_set_grid(grid)
        ctx.debug_service_set_weights(w)
        assert ctx.service_weights() == w
        run_list(ctx, name, G, "run" if grid != 9 else "async", keysel, layout, passes, sz=sz, what=("weights", w0))
        assert ctx.service_weights_used() == w, (grid, ctx.service_weights_used())
