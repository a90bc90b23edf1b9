"""The first mapping of k_verify_batches: every wave finds the batch of its first tile by binary
search over cum[] (batch_find in csrc/hfv_verify_kernels.hip) and steps forward from there.  The
lists of tests/first_map.py put block ranges, and with them the 16 waves' first tiles, on the first
tile of a batch, on its last tile, in its middle and up to 63 batches deep in the list; each list
is compared bit for bit with the CPU checker's verdicts of the base records of tests/tile_deal.py,
about half of whose MACs are corrupted (judged once, on the host; nothing expected here comes from
the library).

Both key rules; batch j's stride alternates between 64 and 72; every batch's bitmap lies between
guard words and is pre-filled with ones, so a dropped word shows, and the empty batches between the
others (which the host drops) must keep their word untouched.

The capped tests set the test build's hfv_debug_batch_grid to 1, 2 and 3 blocks and so run in a
child process on lib/libscionhfv_test.so (conftest.rerun_on_test_build); the real-grid tests run
on the product library."""
import numpy as np
import pytest

import first_map as FM
import scion_hfv as hfv
import test_gpu_tile_deal as G
import tile_deal as TD
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = G.DEV
KEYSELS = (0, 1)

ctx = G.ctx
cap = G.cap


class DevList:
    """A list of tests/first_map.py on the device: every batch gathered from the uploaded base
    into its own stride, and the arena of bitmaps."""

    def __init__(self, name, B, keysel):
        self.name, self.sz = name, FM.sizes(name, B)
        base, s = G.dev_base(keysel), TD.start(name)
        lay = FM.LAYOUT
        self.recs, off = [], 0
        for n, stride in zip(self.sz, FM.strides(self.sz)):
            r = torch.full((max(n, 1), stride), TD.FILLER, dtype=torch.uint8, device=DEV)
            if n:
                i = (torch.arange(n, device=DEV) + (s + off)) % TD.K
                r[:, lay[0]:lay[0] + 8] = base[i, 40:48]
                r[:, lay[1]:lay[1] + 12] = base[i, 48:60]
            self.recs.append((r, stride))
            off += n
        self.arena = G.Arena(self.sz)

    def batches(self):
        return [(r, n, self.arena.bits(j), stride) for j, (n, (r, stride)) in enumerate(zip(self.sz, self.recs))]

    def check(self, passes, what):
        self.arena.check(TD.expected(self.name, self.sz, passes), what)


def run_lists(c, names, B, keysel, passes, what):
    for name in names:
        L = DevList(name, B, keysel)
        c.verify_batches(L.batches())
        L.check(passes, (name, "B=%d" % B) + tuple(what))


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("keysel", KEYSELS)
def test_capped_lists(request, ctx, cap, keysel):
    """Every list under 1, 2 and 3 blocks: the 16 waves of a block find 16 neighbouring tiles."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    G.setup(ctx, keysel, FM.LAYOUT)
    passes = TD.base(keysel)[1]
    for B in (1, 2, 3):
        cap(B)
        run_lists(ctx, FM.NAMES, B, keysel, passes, (keysel,))


@pytest.mark.parametrize("keysel", KEYSELS)
def test_real_grid_lists(ctx, keysel):
    """Every list on one block per CU, on the product library: block k of ones64 starts in batch k."""
    B = cu_count()
    G.setup(ctx, keysel, FM.LAYOUT)
    run_lists(ctx, FM.NAMES, B, keysel, TD.base(keysel)[1], (keysel, "real grid"))


def test_capped_no_key_in_slot_0(request, ctx, cap):
    """KEYSEL_ZERO with slot 0 empty on pairs64 (and the three launches of over130): the fail-closed
    loop starts from the same first mapping.  Every word is 0 and nothing else is written."""
    if rerun_on_test_build(request):
        return
    G.setup(ctx, 0, FM.LAYOUT, slots=range(1, 256))
    for B in (1, 2, 3):
        cap(B)
        run_lists(ctx, ("pairs64", "over130"), B, 0, np.zeros(TD.K, dtype=bool), ("no key",))


def test_real_grid_no_key_in_slot_0(ctx):
    G.setup(ctx, 0, FM.LAYOUT, slots=range(1, 256))
    run_lists(ctx, ("pairs64", "deep"), cu_count(), 0, np.zeros(TD.K, dtype=bool), ("no key", "real grid"))
