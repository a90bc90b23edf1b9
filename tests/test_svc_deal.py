"""tests/svc_deal.py held to itself, to csrc/hfv_internal.h and to the CPU checker (no GPU): the share
model partitions every batch under any weights svc_balance can produce and agrees with svc_cum
compiled from the header, every list's placement is pinned literally, the records are such that
tests/test_gpu_svc_deal.py cannot pass by accident, and its matrix covers what it must."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import orc
import svc_deal as SD
import tile_deal as TD

GRID = 256                        # the MI355X's CUs: the real grid of the GPU legs
BLOCKS = (1, 2, 3, GRID)
CSRC = os.path.join(orc.ROOT, "scion-xdp-br_amd", "csrc")

# (list, G) -> Place(batches, smallest and largest share, every block's largest share exceeds 63 x
# its waves, empty shares, n % 64 of the batches whose tile count is a multiple of G / one less / one
# more, descriptors inline and relayed and the stop's slot under hfv_service_run, the ring wraps);
# counts with its default of 65 batches
PLACEMENT = {
    ("fill", 1): (2, 946, 1906, True, 0, (), (), (), 3, 0, 2, False),
    ("train", 1): (50, 0, 1191, True, 8, (), (), (), 51, 0, 50, False),
    ("edges", 1): (11, 1, 97, False, 0, (), (), (), 12, 0, 11, False),
    ("counts", 1): (65, 1, 3, False, 0, (), (), (), 64, 2, 65, False),
    ("over_ring", 1): (343, 0, 3, False, 43, (), (), (), 64, 280, 87, True),
    ("fewer", 1): (25, 1, 3, False, 0, (), (), (), 26, 0, 25, False),
    ("fill", 2): (1, 1008, 1009, True, 0, (), (1,), (1,), 2, 0, 1, False),
    ("train", 2): (50, 0, 596, False, 40, (), (1, 63), (1, 63), 51, 0, 50, False),
    ("edges", 2): (11, 0, 49, False, 2, (0, 1, 63), (0, 1, 63), (0, 1, 63), 12, 0, 11, False),
    ("counts", 2): (65, 0, 2, False, 33, (), (1,), (1,), 64, 2, 65, False),
    ("over_ring", 2): (343, 0, 2, False, 186, (), (0,), (0,), 64, 280, 87, True),
    ("fewer", 2): (25, 0, 3, False, 22, (), (0, 1, 63), (0, 1, 63), 26, 0, 25, False),
    ("fill", 3): (1, 1008, 1009, True, 0, (), (1,), (), 2, 0, 1, False),
    ("train", 3): (50, 0, 397, False, 80, (1, 63), (), (1,), 51, 0, 50, False),
    ("edges", 3): (11, 0, 33, False, 4, (0, 1, 63), (0, 1, 63), (0, 1, 63), 12, 0, 11, False),
    ("counts", 3): (65, 0, 1, False, 90, (1,), (), (), 64, 2, 65, False),
    ("over_ring", 3): (343, 0, 1, False, 429, (0,), (), (), 64, 280, 87, True),
    ("fewer", 3): (25, 0, 3, False, 37, (), (), (0, 1, 63), 26, 0, 25, False),
    ("fill", 256): (1, 11, 12, False, 0, (), (), (), 2, 0, 1, False),
    ("train", 256): (50, 0, 12, False, 12224, (), (), (), 51, 0, 50, False),
    ("edges", 256): (11, 0, 3, False, 512, (0, 1, 63), (0, 1, 63), (0, 1, 63), 12, 0, 11, False),
    ("counts", 256): (65, 0, 1, False, 16535, (), (), (), 64, 2, 65, False),
    ("over_ring", 256): (343, 0, 1, False, 87208, (), (), (), 64, 280, 87, True),
    ("fewer", 256): (25, 0, 3, False, 4965, (), (63,), (0, 1, 63), 26, 0, 25, False),
}

# run length -> Post(inline, relayed, the stop's slot, the ring wraps, all posted before the launch)
# for hfv_service_run / run_async, submitv on a stopped service, live submits
POSTING = {
    63: ((64, 0, 63, False, True), (63, 1, 63, False, False), (0, 64, 63, False, False)),
    64: ((64, 1, 64, False, True), (64, 1, 64, False, False), (0, 65, 64, False, False)),
    65: ((64, 2, 65, False, True), (64, 2, 65, False, False), (0, 66, 65, False, False)),
    127: ((64, 64, 127, False, True), (64, 64, 127, False, False), (0, 128, 127, False, False)),
    128: ((64, 65, 0, True, False), (64, 65, 0, True, False), (0, 129, 0, True, False)),
    129: ((64, 66, 1, True, False), (64, 66, 1, True, False), (0, 130, 1, True, False)),
}

# weights at and inside the clamp [512, 2048]: equal, the clamp's ends, the weighted leg's pattern
# with both of its w0, and two seeded draws
WEIGHTS = (
    SD.EQUAL, ((512,) * 8, 512), ((2048,) * 8, 2048), ((512,) * 8, 2048), ((2048,) * 8, 512),
    (SD.PATTERN, 512), (SD.PATTERN, 2048),
    ((1999, 513, 2047, 600, 1024, 1025, 2048, 512), 1023), ((700, 701, 1400, 1401, 512, 2048, 900, 1100), 1777),
)
PART_G = (1, 2, 3, 7, 8, 9, 17, 256)


PART_T = tuple(range(1, 3101)) + (5127, 65535, (1 << 20) + 1, (1 << 24) - 1)


@pytest.mark.parametrize("G", PART_G)
def test_shares_partition_every_batch(G):
    """Under every weight set the shares tile [0, T) without gap or overlap, for every T from 1 to
    3100 (past the largest fill) and a few large T; equal weights give the plain T k // G split."""
    T = np.array(PART_T, dtype=np.int64)[:, None]
    for w, w0 in WEIGHTS:
        assert all(SD.CLAMP[0] <= x <= SD.CLAMP[1] for x in w + (w0,))
        cums = [SD.cum(w, w0, k) for k in range(G + 1)]
        assert SD.cum_loop(w, w0, G) == cums                                        # svc_balance's loop
        first = T * np.array(cums[:-1], dtype=np.int64) // cums[-1]                 # [T, k]: share k's first tile
        end = T * np.array(cums[1:], dtype=np.int64) // cums[-1]                    # ... and its end
        assert (first[:, 0] == 0).all() and (end[:, -1] == T[:, 0]).all(), (w, w0)
        assert (first <= end).all() and (end[:, :-1] == first[:, 1:]).all(), (w, w0)
        for t in (1, G, 3026, (1 << 24) - 1):                                        # the model's own shares()
            assert SD.shares(t, G, w, w0) == list(zip((t * np.array(cums[:-1]) // cums[-1]).tolist(),
                                                      (t * np.array(cums[1:]) // cums[-1]).tolist()))
        if (w, w0) == SD.EQUAL:
            k = np.arange(G + 1, dtype=np.int64)
            assert (first == (T * k[:-1] // G)).all() and (end == (T * k[1:] // G)).all()
    assert SD.cum(*SD.EQUAL, G) == G * SD.UNIT


HOST_T = tuple(range(1, 41)) + (63, 64, 65, 127, 128, 129, 255, 256, 257, 946, 2017, 3026, 5127, 65535, (1 << 20) + 1)

HOST_SRC = r"""
#include <stdio.h>
#include <vector>
#include "hfv_internal.h"
using namespace hfv;
static const uint32_t WS[][9] = {%(ws)s};
static const uint64_t GS[] = {%(gs)s};
static const uint64_t TS[] = {%(ts)s};
int main()
{
    for (auto &ws : WS) {
        SvcWeights sw = {};
        for (int x = 0; x < 8; ++x) sw.w[x] = ws[x];
        sw.w0 = ws[8];
        for (uint64_t G : GS) {
            // the host's cum[] loop of svc_balance (hfv_service.cpp), restated
            std::vector<uint64_t> cum(G + 1, 0);
            for (uint64_t k = 0; k < G; ++k) cum[k + 1] = cum[k] + (k ? sw.w[k %% 8] : sw.w0);
            printf("cum");
            for (uint64_t k = 0; k <= G; ++k) {
                if (cum[k] != svc_cum(sw, k)) return 1;
                printf(" %%llu", (unsigned long long)svc_cum(sw, k));
            }
            printf("\n");
            const uint64_t W = svc_cum(sw, G);
            for (uint64_t T : TS) {   // svc_share (hfv_service_kernel.hip): first tile and count
                printf("share");
                for (uint64_t k = 0; k < G; ++k) {
                    const uint64_t t0 = T * svc_cum(sw, k) / W;
                    const uint32_t count = (uint32_t)(T * svc_cum(sw, k + 1) / W - t0);
                    printf(" %%llu+%%u", (unsigned long long)t0, count);
                }
                printf("\n");
            }
        }
    }
    static_assert(kSvcRing == %(ring)d && kSvcInline == %(inline)d && kSvcWeightUnit == %(unit)d, "constants");
    return 0;
}
"""


def test_model_agrees_with_the_header(tmp_path):
    """svc_cum from csrc/hfv_internal.h, compiled into a host program with the host's cum[] loop of
    svc_balance beside it: its prefix sums and the shares the kernel derives from them, printed for
    the same weights, grids and tile counts, equal the Python model's."""
    src = tmp_path / "svc_cum.cpp"
    src.write_text(HOST_SRC % {
        "ws": ", ".join("{%s}" % ", ".join(str(x) for x in w + (w0,)) for w, w0 in WEIGHTS),
        "gs": ", ".join(str(g) for g in PART_G), "ts": ", ".join("%dull" % t for t in HOST_T),
        "ring": SD.RING, "inline": SD.INLINE, "unit": SD.UNIT})
    exe = tmp_path / "svc_cum"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = []
    for w, w0 in WEIGHTS:
        for G in PART_G:
            want.append("cum " + " ".join(str(SD.cum(w, w0, k)) for k in range(G + 1)))
            for T in HOST_T:
                want.append("share " + " ".join("%d+%d" % (a, b - a) for a, b in SD.shares(T, G, w, w0)))
    assert len(got) == len(want) == len(WEIGHTS) * len(PART_G) * (1 + len(HOST_T))
    assert got == want


def test_placement_table():
    got = {(name, G): tuple(SD.placement(SD.sizes(name, G), G)) for G in BLOCKS for name in SD.NAMES}
    assert got == PLACEMENT


def test_posting_table():
    got = {L: tuple(tuple(SD.posting(L, e)) for e in ("run", "stopped", "live")) for L in SD.RUN_LENGTHS}
    assert got == POSTING
    assert all(SD.posting(L, "async") == SD.posting(L, "run") for L in SD.RUN_LENGTHS)


def test_lists_are_what_the_gpu_legs_need():
    """What the tables must show for the legs of tests/test_gpu_svc_deal.py to mean something."""
    P = {k: SD.Place(*v) for k, v in PLACEMENT.items()}
    # fill: by pigeonhole some wave of every block fills its stash inside the one batch
    assert [SD.fill_T(G) for G in (1, 2, 3)] == [946, 2017, 3026]
    for G in (1, 2, 3):
        sz = SD.fill(G)
        assert all(n % 64 == 1 for n in sz) and P["fill", G].fills and SD.tiles(sz[0]) == SD.fill_T(G)
        assert not all(b - a > 63 * SD.waves(k) for k, (a, b) in enumerate(SD.shares(SD.fill_T(G) - 1, G)))
    assert SD.tiles(SD.fill(1)[1]) > 127 * 15            # one block: a wave fills its stash twice
    # train: ragged ends, dozens of small batches with empty ones among them, many empty shares
    for G in BLOCKS:
        sz = SD.train(G)
        assert sz[0] % 64 == 1 and sz[-1] % 64 == 63 and sz.count(0) == 8 and len(sz) == 50
        assert set(sz[1:-1]) == {0, 1, 63, 64, 65, 129} and sum(SD.tiles(n) for n in sz) == SD.big_T(G)
        assert len(sz) + 1 <= SD.INLINE                  # a run grid takes it whole in its arguments
    assert P["train", 2].empty_shares >= 40 and P["train", 3].empty_shares >= 80
    # edges: a tile count on, before and after a multiple of G, each with every n % 64
    for G in (2, 3, GRID):
        p = P["edges", G]
        assert p.on == p.before == p.after == SD.REMS
    for G in BLOCKS:
        assert SD.edges(G)[0] == SD.edges(G)[-1] == 1
    # counts: batches of 1 to 129 records; the stop lands on every edge of the inline array and the ring
    for L in SD.RUN_LENGTHS:
        sz = SD.counts(1, L)
        assert len(sz) == L and min(sz) == 1 and max(sz) == 129
    assert [SD.posting(L, "run").stop_slot for L in SD.RUN_LENGTHS] == [63, 64, 65, 127, 0, 1]
    assert SD.posting(63, "run").relayed == 0 and SD.posting(64, "run").relayed == 1   # stop = inl[63]; first relayed
    assert SD.posting(127, "run").up_front and not SD.posting(128, "run").up_front     # 128: launched mid-post
    # over_ring: the ring wraps twice; fewer: runs of ten and more batches of fewer tiles than blocks
    sz = SD.over_ring(1)
    assert len(sz) == 343 and sz.count(0) == 43 and len(sz) > 2 * SD.RING
    for G in (2, 3, GRID):
        sz, run, best = SD.fewer(G), 0, []
        for n in sz:
            run = run + 1 if SD.tiles(n) < G else 0
            best.append(run)
        assert sorted(best)[-1] >= 12 and sum(1 for i, r in enumerate(best) if r >= 10) >= 4
        assert any(SD.tiles(n) == 1 for n in sz) and any(SD.tiles(n) == G - 1 for n in sz)
    # the largest list is about 200 k records below the real grid, about 330 k on it
    assert max(sum(SD.sizes(name, G)) for G in (1, 2, 3) for name in SD.NAMES) <= 200000
    assert max(sum(SD.sizes(name, GRID)) for name in SD.NAMES) <= 400000


def test_weighted_leg_moves_every_share():
    """The weighted leg's pattern at its grids: of T = 20 G + 7 tiles every share differs from the
    equal split's and none is empty; its train-shaped list has that many tiles."""
    for G in (3, 8, 9, 17, GRID):
        T = SD.weighted_T(G)
        sz = SD.weighted_train(G)
        assert sum(SD.tiles(n) for n in sz) == T and sz[0] % 64 == 1 and sz[-1] % 64 == 63 and sz.count(0) == 2
        for w0 in (512, 2048):
            sh, eq = SD.shares(T, G, SD.PATTERN, w0), SD.shares(T, G)
            assert all(a < b for a, b in sh) and not any(x == y for x, y in zip(sh, eq)), (G, w0)


@pytest.mark.parametrize("keysel", [0, 1])
def test_no_word_can_stand_in(keysel):
    """Within every list the GPU legs run, the expected words of all full tiles are pairwise
    distinct and none is 0 or all ones (tests/tile_deal.py)."""
    _, passes = TD.base(keysel)
    for G in BLOCKS:
        for name in SD.NAMES:
            if name != "counts":
                TD.assert_no_word_can_stand_in(SD.tag(name), SD.sizes(name, G), passes)
    for L in SD.RUN_LENGTHS:
        TD.assert_no_word_can_stand_in(SD.tag("counts", L), SD.counts(1, L), passes)
    for G in (3, 8, 9, 17, GRID):
        TD.assert_no_word_can_stand_in(SD.tag("train"), SD.weighted_train(G), passes)


def test_matrix_covers_every_list_and_entry_point_on_every_grid():
    """The only selection in tests/test_gpu_svc_deal.py is its matrix: every list and every entry
    point meets every grid, both key rules and both layouts meet every grid, and the GPU file's
    docstring states the matrix row by row."""
    M = SD.MATRIX
    assert len(set(M)) == len(M)
    assert {(name, G) for name, G, *_ in M} == set(itertools.product(SD.NAMES, SD.GRIDS))
    assert {(e, G) for _, G, e, *_ in M} == set(itertools.product(SD.ENTRIES, SD.GRIDS))
    assert {(ks, G) for _, G, _, ks, _, _ in M} == set(itertools.product((0, 1), SD.GRIDS))
    assert {(ly, G) for _, G, _, _, ly, _ in M} == set(itertools.product((0, 1), SD.GRIDS))
    assert all((L in SD.RUN_LENGTHS) == (name == "counts") for name, _, _, _, _, L in M)
    doc = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_svc_deal.py")).read().split('"""')[1]
    rows = [line.split() for line in doc.splitlines() if line.startswith("    G=")]
    stated = set()
    for row in rows:
        G = int(row[0][2:])
        for cell in row[1:]:
            name, entry, ks, ly = cell.split("/")
            name, _, L = name.partition(":")
            stated.add((name, G, entry, int(ks[1:]), int(ly[1:]), int(L) if L else None))
    assert stated == set(M)
