"""The first mapping of k_verify_batches restated in plain Python, and batch lists that stress it.

TEST INFRASTRUCTURE ONLY.

The model (on top of tests/tile_deal.py's: launches, cum[], block ranges).  Wave w of block k
takes tile b0 + w first, b0 the start of the block's range (a wave past the range maps the range's
last tile and verifies nothing), and finds that tile's batch by binary search over cum[0..nb]
(batch_find in csrc/hfv_verify_kernels.hip): the j with cum[j] <= g < cum[j + 1].  cum[] is strictly
increasing, since the host drops empty batches.  Every later tile of the wave is mapped by a
forward step from there.

The lists (every size a function of the block count B, as in tests/tile_deal.py):

  ones64     64 batches of one record: at 64 blocks and more block k's first tile is batch k, so
             every j is found by some block
  pairs64    64 batches of 65 records: two tiles each, the second ragged
  deep       63 one-tile batches in front of one batch of 17 B tiles: the last block starts deep
             in the list, and in the last batch's middle
  longfirst  a first batch of 4 B + 3 tiles, longer than block 0's range: blocks 1.. start in the
             middle of batch 0
  nb1, nb2, nb3, nb63   lists of that many non-empty batches, of 1, 2 and 3 tiles (ragged ends)
  over130    130 non-empty batches: three launches (64, 64, 2)
Every list but nb1 carries empty batches between the others (sizes()), which the host drops."""
import tile_deal as TD

NAMES = ("ones64", "pairs64", "deep", "longfirst", "nb1", "nb2", "nb3", "nb63", "over130")
STRIDES = (64, 72)                # batch j's stride, alternating (layout 40/48)
LAYOUT = (40, 48)
MAX_PROBES = 7                    # the issue's bound; nb <= 64 needs 6


def batch_find(cum, nb, g):
    """(j, scalar loads): the search as the kernel does it."""
    lo, length, probes = 0, nb, 0        # cum[lo] <= g < cum[lo + length]
    while length > 1:
        half = length >> 1
        probes += 1
        if g >= cum[lo + half]:
            lo += half
            length -= half
        else:
            length = half
    return lo, probes


def batch_scan(cum, g):
    """The forward scan from batch 0 that batch_find replaces."""
    j = 0
    while g >= cum[j + 1]:
        j += 1
    return j


def live(B):
    """name -> the non-empty batches' sizes."""
    rag = lambda i: TD.n_of(1 + i % 3, TD.REMS[i % 3])   # noqa: E731  1, 2, 3 tiles; n % 64 = 0, 1, 63
    return {
        "ones64": [1] * 64,
        "pairs64": [65] * 64,
        "deep": [(1, 63, 64)[i % 3] for i in range(63)] + [TD.n_of(17 * B, 63)],
        "longfirst": [TD.n_of(4 * B + 3, 63), 1, 65, 64, TD.n_of(B, 1)],
        "nb1": [TD.n_of(2 * B + 1, 1)],
        "nb2": [TD.n_of(B + 1, 63), TD.n_of(B, 1)],
        "nb3": [TD.n_of(B, 0), 1, TD.n_of(B + 2, 63)],
        "nb63": [rag(i) for i in range(63)],
        "over130": [rag(i + 1) for i in range(130)],
    }


def sizes(name, B):
    """The list as the caller passes it: an empty batch in front of every fifth one, after the
    first batch and at the end (none in nb1)."""
    out = []
    for i, n in enumerate(live(B)[name]):
        if name != "nb1" and (i % 5 == 2 or i == 1):
            out.append(0)
        out.append(n)
    return out if name == "nb1" else out + [0]


def strides(sz):
    return [STRIDES[j % 2] for j in range(len(sz))]


def first_maps(sz, B):
    """Per launch: (deal, [(block, wave, tile, j)]) for every wave whose first tile is in its
    block's range."""
    out = []
    for launch in TD.launches(sz):
        d = TD.deal(launch, B)
        maps = []
        for k, (a, b) in enumerate(d.ranges):
            for w in range(16):
                if a + w < b:
                    maps.append((k, w, a + w, batch_scan(d.cum, a + w)))
        out.append((d, maps))
    return out


def range_starts(sz, B):
    """Where block ranges begin within their batches, over all launches: a set of "first"
    (a batch's first tile, of a batch of two tiles and more), "last" (its last tile, likewise),
    "middle" (neither), "only" (a one-tile batch)."""
    kinds = set()
    for d, _ in first_maps(sz, B):
        for a, _ in d.ranges:
            j = batch_scan(d.cum, a)
            lo, hi = d.cum[j], d.cum[j + 1]
            kinds.add("only" if hi - lo == 1 else "first" if a == lo else "last" if a == hi - 1 else "middle")
    return kinds
