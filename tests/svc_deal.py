"""The tile dealing of k_verify_service restated in plain integers, batch lists that stress it, and
the matrix of list x grid x entry point that tests/test_gpu_svc_deal.py runs.  The records, their
verdicts (the CPU checker's, judged once) and the expected words come from tests/tile_deal.py.

TEST INFRASTRUCTURE ONLY.

The model (hfv_internal.h, hfv_service_kernel.hip, hfv_service.cpp).  Block j of a grid of G weighs
w[j % 8], block 0 weighs w0; cum(w, w0, k) sums the weights of blocks 0 .. k - 1 and W = cum(G).
Block k's share of a batch of T tiles is [T cum(k) // W, T cum(k + 1) // W): every batch is split
on its own, an empty batch (n = 0) is posted like any other (a ticket, a slot, every share empty).
Batch b sits in ring slot b % 128.  Batches posted before the launch travel in the kernel
arguments, up to 64 of them; the rest are relayed.  hfv_service_run posts the batches and a stop
descriptor behind them, and launches first once the ring is full (128 posted).  Block 0 verifies
with 15 waves (its 16th relays), every other block with 16.  Which wave claims which tile is
decided at run time and is not modelled.

The lists, each a function of the grid G:

  fill       one ragged batch (n % 64 = 1) so large that every block's share exceeds 63 x its
             waves: some wave fills its 64-word stash inside the batch.  G = 1 adds a batch above
             127 x 15 tiles (two fills).  Above 3 blocks the size stays that of 3 blocks (filling a
             stash on 256 blocks takes 2^24 records), so there it is one ragged batch and no more.
  train      a ragged large batch, 40 batches cycling n = 1, 63, 64, 65, 129 with 8 empty ones
             among them, a ragged large batch; T tiles in all (default max(2048, 20 G + 7))
  edges      every batch is split on its own, so the edge is a batch's tile count against G: T a
             multiple of G (every share start T k / G exact: the boundary ON them), one tile less
             (BEFORE) and one more (AFTER), each ending on n % 64 = 0, 1 and 63; one-record batches
             first and last
  counts     L batches of 1 .. 129 records, L = 63, 64, 65, 127, 128, 129: with the stop behind
             them these put the stop on every edge of the inline array and the ring
  over_ring  300 small batches with 43 empty ones between them
  fewer      batches of fewer tiles than blocks (T = 1 among them) in runs of 12 and 10, between
             batches of 2 G + 1 tiles

placement() says where a list falls; tests/test_svc_deal.py pins it literally."""
import collections

import tile_deal as TD

RING = 128                        # kSvcRing
INLINE = 64                       # kSvcInline
UNIT = 1024                       # kSvcWeightUnit
CLAMP = (512, 2048)               # what svc_balance can produce
EQUAL = ((UNIT,) * 8, UNIT)
PATTERN = (512, 2048, 1024, 777, 1500, 2048, 512, 1300)   # the weighted leg's w; w0 = 512 and 2048
REMS = TD.REMS
NAMES = ("fill", "train", "edges", "counts", "over_ring", "fewer")
RUN_LENGTHS = (63, 64, 65, 127, 128, 129)
ENTRIES = ("run", "async", "live", "stopped")
GRIDS = (1, 2, 3, 0)              # hfv_service_set_grid's argument; 0: one block per CU

Place = collections.namedtuple("Place", "batches share_min share_max fills empty_shares on before after "
                                        "inline relayed stop_slot wraps")
Post = collections.namedtuple("Post", "inline relayed stop_slot wraps up_front")


# ---- the model ----------------------------------------------------------------------------------

def cum(w, w0, k):
    """svc_cum: the weights of blocks 0 .. k - 1."""
    if k == 0:
        return 0
    return (k // 8) * sum(w) + sum(w[:k % 8]) - w[0] + w0


def cum_loop(w, w0, G):
    """The host's cum[] loop in svc_balance."""
    c = [0]
    for k in range(G):
        c.append(c[-1] + (w[k % 8] if k else w0))
    return c


def shares(T, G, w=EQUAL[0], w0=EQUAL[1]):
    """Every block's [first tile, end) of a batch of T tiles."""
    W = cum(w, w0, G)
    return [(T * cum(w, w0, k) // W, T * cum(w, w0, k + 1) // W) for k in range(G)]


def waves(k):
    """Waves of block k that verify."""
    return 15 if k == 0 else 16


def tiles(n):
    return (n + 63) // 64


def posting(count, entry):
    """Where `count` batches travel for an entry point: descriptors in the kernel arguments,
    descriptors relayed (the stop included, whoever posts it), the stop's ring slot, whether the
    ring wraps, and whether batches and stop are all in the ring before the grid starts."""
    if entry in ("run", "async"):     # batches and the stop, launched once RING are posted
        posted = min(count + 1, RING)
    elif entry == "stopped":          # submitv on a stopped service: the batches alone; service_stop posts the stop
        posted = min(count, RING)
    else:                             # live: the grid is started first
        posted = 0
    inline = min(posted, INLINE)
    return Post(inline, count + 1 - inline, count % RING, count + 1 > RING, entry in ("run", "async") and count < RING)


def placement(sz, G, entry="run", w=EQUAL[0], w0=EQUAL[1]):
    """Where a list's batches fall against the shares of G blocks, and how `entry` posts it."""
    most = [0] * G
    sizes, empty = [], 0
    at = {0: set(), -1: set(), 1: set()}
    for n in sz:
        T = tiles(n)
        for k, (a, b) in enumerate(shares(T, G, w, w0)):
            most[k] = max(most[k], b - a)
            sizes.append(b - a)
            empty += a == b
        if T > 2 and G > 1:
            if T % G == 0:
                at[0].add(n % 64)
            if T % G == G - 1:
                at[-1].add(n % 64)
            if T % G == 1:
                at[1].add(n % 64)
    t = lambda s: tuple(sorted(s))   # noqa: E731
    p = posting(len(sz), entry)
    return Place(len(sz), min(sizes), max(sizes), all(most[k] > 63 * waves(k) for k in range(G)), empty,
                 t(at[0]), t(at[-1]), t(at[1]), p.inline, p.relayed, p.stop_slot, p.wraps)


# ---- the lists ----------------------------------------------------------------------------------

n_of = TD.n_of


def fill_T(G):
    """The fewest tiles of which every one of G blocks gets more than 63 x its waves (equal weights)."""
    T = G * 63 * 15
    while not all(b - a > 63 * waves(j) for j, (a, b) in enumerate(shares(T, G))):
        T += 1
    return T


def fill(G):
    G = min(G, 3)
    return [n_of(fill_T(G), 1)] + ([n_of(127 * 15 + 1, 1)] if G == 1 else [])


def big_T(G):
    return max(2048, 20 * G + 7)


def train(G, T=None, k=40):
    T = big_T(G) if T is None else T
    mid, small = [], 0
    for i in range(k):
        if i % 5 == 2:
            mid.append(0)
        mid.append((1, 63, 64, 65, 129)[i % 5])
        small += tiles(mid[-1])
    first = 2 * (T - small) // 5
    return [n_of(first, 1)] + mid + [n_of(T - small - first, 63)]


def edges(G):
    q = max(1, -(-48 // G))
    sz = [1]
    for i, (d, r) in enumerate((d, r) for d in (0, -1, 1) for r in REMS):
        sz.append(n_of(q * (1, 2, 1)[(i + i // 3) % 3] * G + d, r))
    return sz + [1]


def counts(G, L=65):
    return [(1, 63, 64, 65, 129, 2, 128, 127)[i % 8] for i in range(L)]


def over_ring(G):
    sz = []
    for i in range(300):
        if i % 7 == 3:
            sz.append(0)
        sz.append(n_of(1 + i % 3, REMS[(i + 1) % 3]))
    return sz


def fewer(G):
    cap = lambda t: max(1, min(G - 1, t))   # noqa: E731
    big = 2 * G + 1
    run_a = [(1, 63, 64)[i % 3] for i in range(12)]                       # T = 1
    run_b = [n_of(cap(t), REMS[i % 3]) for i, t in enumerate((2, 3, G - 1, 1, G // 2, 2, 5, 1, G - 1, 3))]
    return [n_of(big, 1)] + run_a + [n_of(big, 63)] + run_b + [n_of(big, 0)]


def sizes(name, G, L=None):
    if name == "counts":
        return counts(G, 65 if L is None else L)
    return {"fill": fill, "train": train, "edges": edges, "over_ring": over_ring, "fewer": fewer}[name](G)


def tag(name, L=None):
    """The list's name in tests/tile_deal.py's seeded starts (TD.start, TD.expected)."""
    return "svc_" + name + ("" if L is None else str(L))


def weighted_T(G):
    return 20 * G + 7


def weighted_train(G):
    """The weighted leg's list: train's shape with 10 small batches, 20 G + 7 tiles in all."""
    return train(G, weighted_T(G), 10)


# ---- the matrix ---------------------------------------------------------------------------------

# (list, grid, entry point, keysel, layout number in TD.LAYOUTS, run length of counts).  The list of
# column i and the grid of row j go through entry point (i + j) % 4, so that every list meets every
# grid and, six lists to four entry points, every entry point meets every grid.
MATRIX = (
    ("fill", 1, "run", 0, 0, None), ("train", 1, "async", 1, 1, None), ("edges", 1, "live", 0, 1, None),
    ("counts", 1, "stopped", 1, 0, 127), ("over_ring", 1, "run", 1, 1, None), ("fewer", 1, "async", 0, 0, None),
    ("fill", 2, "async", 1, 1, None), ("train", 2, "live", 0, 0, None), ("edges", 2, "stopped", 1, 0, None),
    ("counts", 2, "run", 0, 1, 64), ("over_ring", 2, "async", 0, 0, None), ("fewer", 2, "live", 1, 1, None),
    ("fill", 3, "live", 0, 1, None), ("train", 3, "stopped", 1, 0, None), ("edges", 3, "run", 1, 1, None),
    ("counts", 3, "async", 0, 0, 128), ("over_ring", 3, "live", 1, 0, None), ("fewer", 3, "stopped", 0, 1, None),
    ("fill", 0, "stopped", 1, 0, None), ("train", 0, "run", 0, 1, None), ("edges", 0, "async", 0, 0, None),
    ("counts", 0, "live", 1, 1, 65), ("over_ring", 0, "stopped", 0, 1, None), ("fewer", 0, "run", 1, 0, None),
)
