"""tests/tile_deal.py held to itself and to the CPU checker (no GPU): the dealing model partitions
the tiles, every list's placement against the block ranges is pinned literally, and the records
are such that tests/test_gpu_tile_deal.py cannot pass by accident."""
import numpy as np
import pytest

import hf_bits as HB
import scion_hfv as hfv
import tile_deal as TD

CAPS = (1, 2, 3)
GRID = 256                        # the MI355X's CUs: the real grid of the GPU legs
BLOCKS = CAPS + (GRID,)

# (list, B) -> Place(launches, most batches inside one block range, n % 64 of the batches ending
# on / one tile before / one tile after a range start, ranges ending on a partial tile, ranges
# ending on a one-record batch before the launch's end, the launches' first and last batches have
# one record, tiles per block min and max); B = 304 shows that the lists follow B
PLACEMENT = {
    ("train", 1): (1, 42, (), (), (), 1, 0, False, False, 2048, 2048),
    ("edges", 1): (1, 3, (), (), (), 1, 0, True, True, 2048, 2048),
    ("over64", 1): (3, 64, (), (), (), 1, 0, False, False, 45, 667),
    ("single", 1): (1, 1, (), (), (), 1, 0, False, False, 2048, 2048),
    ("just16", 1): (1, 3, (), (), (), 1, 0, False, False, 17, 17),
    ("just1", 1): (1, 2, (), (), (), 1, 0, True, True, 2, 2),
    ("just2", 1): (1, 1, (), (), (), 1, 0, True, True, 1, 1),
    ("train", 2): (1, 42, (), (), (), 1, 0, False, False, 1024, 1024),
    ("edges", 2): (1, 3, (1,), (0,), (63,), 2, 1, True, True, 1024, 1024),
    ("over64", 2): (3, 33, (1,), (0,), (0,), 2, 1, False, False, 22, 334),
    ("single", 2): (1, 1, (), (), (), 1, 0, False, False, 1024, 1024),
    ("just16", 2): (1, 3, (), (), (), 1, 0, False, False, 16, 17),
    ("just1", 2): (1, 2, (63,), (), (1,), 2, 0, False, True, 1, 2),
    ("just2", 2): (1, 2, (63,), (), (1,), 2, 0, False, True, 1, 2),
    ("train", 3): (1, 42, (), (), (), 1, 0, False, False, 682, 683),
    ("edges", 3): (1, 3, (1, 63), (0, 1), (0, 63), 3, 1, True, True, 682, 683),
    ("over64", 3): (3, 22, (0, 1, 63), (0, 1), (1, 63), 3, 1, False, False, 15, 223),
    ("single", 3): (1, 1, (), (), (), 1, 0, False, False, 682, 683),
    ("just16", 3): (1, 3, (), (), (), 1, 0, False, False, 16, 17),
    ("just1", 3): (1, 1, (1, 63), (63,), (1,), 3, 1, False, False, 1, 2),
    ("just2", 3): (1, 2, (1,), (63,), (63,), 2, 1, False, False, 1, 2),
    ("train", 256): (1, 14, (1,), (0,), (1,), 3, 0, False, False, 20, 21),
    ("edges", 256): (1, 2, (0, 1, 63), (0, 1, 63), (0, 1, 63), 5, 2, True, True, 20, 21),
    ("over64", 256): (3, 2, (0, 1, 63), (0, 1, 63), (0, 1, 63), 58, 28, False, False, 1, 18),
    ("single", 256): (1, 1, (), (), (), 1, 0, False, False, 20, 21),
    ("just16", 256): (1, 3, (), (), (), 1, 0, False, False, 16, 17),
    ("just1", 256): (1, 1, (1, 63), (1, 63), (1, 63), 3, 1, False, False, 1, 2),
    ("just2", 256): (1, 2, (1,), (63,), (63,), 2, 1, False, False, 1, 2),
    ("train", 304): (1, 14, (1,), (0,), (1,), 3, 0, False, False, 20, 21),
    ("edges", 304): (1, 2, (0, 1, 63), (0, 1, 63), (0, 1, 63), 5, 2, True, True, 20, 21),
    ("over64", 304): (3, 2, (0, 1, 63), (0, 1, 63), (0, 1, 63), 60, 28, False, False, 1, 18),
    ("single", 304): (1, 1, (), (), (), 1, 0, False, False, 20, 21),
    ("just16", 304): (1, 3, (), (), (), 1, 0, False, False, 16, 17),
    ("just1", 304): (1, 1, (1, 63), (1, 63), (1, 63), 3, 1, False, False, 1, 2),
    ("just2", 304): (1, 2, (1,), (63,), (63,), 2, 1, False, False, 1, 2),
}


@pytest.mark.parametrize("B", BLOCKS + (304,))
def test_block_ranges_partition_the_tiles(B):
    for name in TD.NAMES:
        sz = TD.sizes(name, B)
        ls = TD.launches(sz)
        assert [i for l in ls for i, _ in l] == [i for i, n in enumerate(sz) if n]
        assert all(0 < len(l) <= TD.KBATCH for l in ls) and all(len(l) == TD.KBATCH for l in ls[:-1])
        for launch in ls:
            d = TD.deal(launch, B)
            assert d.T == sum((n + 63) // 64 for n in d.n) and d.G == min(d.T, B) == len(d.ranges)
            assert d.ranges[0][0] == 0 and d.ranges[-1][1] == d.T
            assert all(a < b for a, b in d.ranges), "an empty block range"
            assert all(p[1] == q[0] for p, q in zip(d.ranges, d.ranges[1:]))


def test_placement_table():
    got = {(name, B): tuple(TD.placement(TD.sizes(name, B), B)) for B in BLOCKS + (304,) for name in TD.NAMES}
    assert got == PLACEMENT


def test_lists_are_what_the_gpu_legs_need():
    """What the table must show for the legs of tests/test_gpu_tile_deal.py to mean something."""
    P = {k: TD.Place(*v) for k, v in PLACEMENT.items()}
    for B in CAPS:
        assert TD.deal(TD.launches(TD.train(B))[0], B).T >= 2048
        assert P["train", B].most_batches >= 40          # a wave's claims jump over whole batches
        assert P["single", B].tiles_max >= 64 * 16 // B  # one block: every wave flushes a full stash
        assert TD.deal(TD.launches(TD.over64(B))[0], B).T >= 17 * B
    assert P["train", 1].tiles_max >= 64 * 16            # 64 tiles and more per wave on average
    for B in BLOCKS:
        sz = TD.over64(B)
        assert sum(1 for n in sz if n) == 150 and sz.count(0) == 20 and P["over64", B].launches == 3
        assert TD.deal(TD.launches(sz)[0], B).T >= 17 * B
        assert [TD.deal(TD.launches(TD.sizes(n, B))[0], B).T for n in ("just16", "just1", "just2")] == \
            [16 * B + 1, B + 1, 2 * B - 1]
        assert TD.single(B)[0] % 64 == 1 and TD.single(B)[0] >= 64 * 2048 - 63
        assert all(n % 64 in TD.REMS or n in (65, 129) for name in TD.NAMES for n in TD.sizes(name, B))
        assert sum(TD.sizes("train", B)) <= 400000 and sum(TD.sizes("edges", B)) <= 400000
    assert (P["just16", GRID].tiles_min, P["just16", GRID].tiles_max) == (16, 17)
    # edges: with two or more ranges a boundary on, before and after a start; with three or more
    # every n % 64 among them; a one-record batch first, last and at the end of a range
    for B in (2, 3, GRID):
        p = P["edges", B]
        assert p.on and p.before and p.after and p.one_ends_range >= 1 and p.one_first and p.one_last
    for B in (3, GRID):
        p = P["edges", B]
        assert set(p.on) | set(p.before) | set(p.after) == set(TD.REMS)
    assert P["edges", GRID].on == P["edges", GRID].before == P["edges", GRID].after == TD.REMS
    assert TD.deal(TD.launches(TD.train(GRID))[0], GRID).T == 20 * GRID + 7


@pytest.mark.parametrize("keysel", [0, 1])
def test_base_verdicts_cannot_hide_a_failure(keysel):
    """On the checker's verdicts alone: about half of the base passes, and within every list (at
    the block counts the GPU legs run) the expected words of all full tiles are pairwise distinct
    and none is 0 or all ones -- a word taken from any other tile, a dropped word (the pre-fill)
    or a zeroed one cannot pass."""
    _, passes = TD.base(keysel)
    assert 0.4 < passes.mean() < 0.6
    for B in BLOCKS:
        for name in TD.NAMES:
            TD.assert_no_word_can_stand_in(name, TD.sizes(name, B), passes)


@pytest.mark.parametrize("keysel", [0, 1])
def test_relaid_records_keep_their_verdicts(keysel):
    recs, passes = TD.base(keysel)
    for layout, strides in TD.LAYOUTS.items():
        for stride in strides:
            r = TD.relay(recs, layout, stride)
            assert r.shape == (TD.K, stride)
            got = TD.judge(HB.at_default_offsets(r, layout + (stride,)), keysel, stride=stride, n=TD.K)
            assert np.array_equal(got, passes), (layout, stride)
    # the partial key table of the GPU leg: the records of odd slots fail, and some of each kind exist
    if keysel:
        part = TD.judge(recs, 1, valid=HB.partial_valid())
        odd = HB.slots(recs, (40, 48, 64)) % 2 == 1
        assert not part[odd].any() and np.array_equal(part[~odd], passes[~odd])
        assert passes[odd].sum() > TD.K // 8 and part.sum() > TD.K // 8


def test_expected_words_follow_the_list():
    _, passes = TD.base(0)
    sz = TD.sizes("over64", 2)
    idx = TD.index("over64", sz)
    assert idx[0] == TD.start("over64") and len(idx) == sum(sz) and idx.max() < TD.K
    exp = TD.expected("over64", sz, passes)
    assert [e is None for e in exp] == [n == 0 for n in sz]
    off = sum(sz[:9])
    assert hfv.bits_to_bool(exp[9], sz[9]).tolist() == passes[(TD.start("over64") + off + np.arange(sz[9])) % TD.K].tolist()
    assert all(int(e[-1]) >> (n % 64 or 64) == 0 for e, n in zip(exp, sz) if n)   # no bit at or past n
    assert TD.strides(sz, (0, 8))[:4] == [24, 32, 40, 24]


def test_frames_carry_the_records():
    """The template frame parses (status 0) with a base record's fields in place of its own."""
    recs, _ = TD.base(0)
    fr, length = TD.frames(recs[:300])
    assert fr.shape[1] % 8 == 0 and fr.shape[1] >= max(64, length)
    for i in (0, 1, 150, 299):
        status, inf, hf = hfv.frame_extract(bytes(fr[i, :length]))
        assert status == 0 and inf == recs[i, 40:48].tobytes() and hf == recs[i, 48:60].tobytes()
