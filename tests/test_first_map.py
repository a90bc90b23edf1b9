"""tests/first_map.py checked on the host: the binary search of k_verify_batches' first mapping
against the forward scan it replaces, and where the lists of tests/test_gpu_first_map.py put the
block ranges.  No GPU."""
import numpy as np
import pytest

import first_map as FM
import tile_deal as TD


def test_search_equals_scan_on_random_lists():
    rng = np.random.default_rng(0xF1A5)
    for nb in list(range(1, 65)) * 3:
        cum = [0] + list(np.cumsum(rng.integers(1, 1 << int(rng.integers(1, 20)), nb)))
        total = cum[-1]
        probe = {0, total - 1}
        for j in range(nb):
            probe |= {cum[j], cum[j + 1] - 1}
        probe |= set(int(g) for g in rng.integers(0, total, 32))
        worst = 0
        for g in probe:
            j, probes = FM.batch_find(cum, nb, g)
            assert cum[j] <= g < cum[j + 1], (nb, g)
            assert j == FM.batch_scan(cum, g), (nb, g)
            worst = max(worst, probes)
        assert worst <= FM.MAX_PROBES
        assert worst <= max(1, nb - 1).bit_length()


def test_search_finds_every_batch_of_a_full_list():
    cum = list(range(65))                # 64 one-tile batches
    assert [FM.batch_find(cum, 64, g)[0] for g in range(64)] == list(range(64))
    assert max(FM.batch_find(cum, 64, g)[1] for g in range(64)) == 6


@pytest.mark.parametrize("B", (1, 2, 3, 256))
def test_lists(B):
    """What the lists are built for, at the capped grids and at 256 blocks."""
    counts = {"ones64": 64, "pairs64": 64, "deep": 64, "longfirst": 5, "nb1": 1, "nb2": 2, "nb3": 3, "nb63": 63,
              "over130": 130}
    for name in FM.NAMES:
        sz = FM.sizes(name, B)
        assert sum(1 for n in sz if n) == counts[name], name
        assert (0 in sz) == (name != "nb1"), name
        assert len(TD.launches(sz)) == (3 if name == "over130" else 1), name
        for d, maps in FM.first_maps(sz, B):
            for _, _, g, j in maps:          # the search agrees with the scan on every wave's first tile
                assert FM.batch_find(d.cum, len(d.n), g)[0] == j
    # every batch of the full lists is some wave's first mapping, at any grid
    for name in ("ones64", "pairs64"):
        (d, maps), = FM.first_maps(FM.sizes(name, B), B)
        if B >= 4:
            assert {j for _, _, _, j in maps} == set(range(64)), name
    # the last block of `deep` starts in the last batch's middle, 63 batches deep (48 deep at 2 blocks)
    (d, maps), = FM.first_maps(FM.sizes("deep", B), B)
    a = d.ranges[-1][0]
    if B > 2:
        assert FM.batch_scan(d.cum, a) == 63 and d.cum[63] < a < d.T - 1
    elif B == 2:
        assert FM.batch_scan(d.cum, a) == 48
    # the first batch of `longfirst` is longer than block 0's range
    (d, _), = FM.first_maps(FM.sizes("longfirst", B), B)
    if B > 1:
        assert d.cum[1] > d.ranges[0][1] and FM.batch_scan(d.cum, d.ranges[1][0]) == 0


def test_block_ranges_begin_everywhere_in_a_batch():
    """At 256 blocks the lists begin block ranges on a batch's first tile, its last tile, in its
    middle and on one-tile batches; so do the capped grids taken together."""
    kinds = set()
    for name in FM.NAMES:
        kinds |= FM.range_starts(FM.sizes(name, 256), 256)
    assert kinds == {"first", "last", "middle", "only"}
    kinds = set()
    for B in (2, 3):
        for name in FM.NAMES:
            kinds |= FM.range_starts(FM.sizes(name, B), B)
    assert kinds == {"first", "last", "middle", "only"}
