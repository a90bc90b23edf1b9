"""tests/br_deal.py held to itself, to csrc/hfv_br_kernel.hip and to the CPU checker (no GPU): the
dealing model gives every tile to one wave, the placement the GPU legs rely on is pinned literally,
the block and window constants are the kernel's, and the corpus is such that
tests/test_gpu_br_deal.py cannot pass by accident; the checker's results on the 5157-frame corpus
are held against the reference program where it is built and against tests/golden/br_deal.npz
everywhere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import br_deal as BD
import br_shift as S
import br_topo as T
import orc

GRID = 256                        # the MI355X's CUs: the real grid of the GPU legs
REAL = BD.real_size(GRID)
SIZES = BD.EDGE_SIZES + tuple(BD.deal_size(b) for b in BD.CAPS) + (REAL,)
CSRC = os.path.join(orc.ROOT, "scion-xdp-br_amd", "csrc")


# ---- the model ----------------------------------------------------------------------------------

def test_sizes_are_what_the_issue_of_dealing_needs():
    assert [BD.deal_size(b) for b in BD.CAPS] == [5157, 10277, 15397]
    assert REAL == 281381 and BD.tiles(REAL) == 16 * GRID + 301 and REAL % 64 == 37
    assert BD.tiles(1024) == BD.WAVES                    # one round of one block
    assert REAL * BD.DIRECT_SLOT < 80e6                  # the largest buffer of the GPU legs


@pytest.mark.parametrize("split", [0, BD.SPLIT])
@pytest.mark.parametrize("cap", [1, 2, 3, 0], ids=["grid1", "grid2", "grid3", "real"])
@pytest.mark.parametrize("variant", BD.VARIANTS)
def test_every_tile_has_one_owner(variant, cap, split):
    for n in SIZES:
        own = BD.owners(n, variant, GRID, cap, split)
        assert len(own) == sum(BD.tiles(m) for _, m in BD.pieces(n, GRID, split)), n
        assert (own == 1).all(), (n, variant, cap, split, np.nonzero(own != 1)[0][:8])
        ps = BD.pieces(n, GRID, split)
        assert ps[0][0] == 0 and sum(m for _, m in ps) == n and all(a + m == b for (a, m), (b, _) in zip(ps, ps[1:]))
        assert all(m == split for _, m in ps[:-1]) and (len(ps) == 1 or 0 < ps[-1][1] <= split)


@pytest.mark.parametrize("cap", [1, 2, 3, 0], ids=["grid1", "grid2", "grid3", "real"])
def test_staged_blocks_draw_their_tiles_plus_16(cap):
    for n in SIZES:
        T_, G = BD.tiles(n), BD.grid(n, GRID, cap)
        deal = BD.staged_deal(T_, G)
        assert [r for r, _, _ in deal] == BD.block_ranges(T_, G)
        assert deal[0][0][0] == 0 and deal[-1][0][1] == T_
        for (tb0, tb1), draws, mine in deal:
            assert draws == tb1 - tb0 + BD.WAVES
            assert sorted(t for ts in mine for t in ts) == list(range(tb0, tb1))
            assert all(ts == sorted(ts) for ts in mine)


def test_grid_and_split_literals():
    assert [BD.grid(n, 256) for n in (0, 1, 64, 65, 1024, 16384, 16385, REAL)] == [1, 1, 1, 2, 16, 256, 256, 256]
    assert [BD.grid(REAL, 256, cap) for cap in (0, 1, 2, 3, 300)] == [256, 1, 2, 3, 256]
    assert BD.grid(65, 256, 3) == 2 and BD.grid(1, 256, 3) == 1          # the cap never raises a grid
    assert BD.grid(REAL, 304) == 304
    assert BD.split_cap(256) == (0xFFFFFFFF // 256 - 128) * 256 == 4294934272   # out of reach of any test
    assert BD.split_cap(256, 1000) == 1000 and BD.split_cap(1, 0, 2048) == 0xFFFFFFFF // 2048 - 128
    assert BD.pieces(10277, 256, 1000)[-1] == (10000, 277) and len(BD.pieces(10277, 256, 1000)) == 11
    assert BD.pieces(10277, 256, 1000, counted=False) == [(0, 10277)]   # a call without counters is never split
    assert BD.pieces(1000, 256, 1000) == [(0, 1000)] and BD.pieces(1001, 256, 1000) == [(0, 1000), (1000, 1)]


def test_placement_table():
    """Where the dealing sizes and the real-grid size put their tiles."""
    n1, n2, n3 = (BD.deal_size(b) for b in BD.CAPS)
    assert (BD.tiles(n1), BD.tiles(n2), BD.tiles(n3)) == (81, 161, 241)
    assert BD.block_ranges(81, 1) == [(0, 81)]
    assert BD.block_ranges(161, 2) == [(0, 80), (80, 161)]
    assert BD.block_ranges(241, 3) == [(0, 80), (80, 160), (160, 241)]
    # the direct deal: one wave runs six tiles, every other five
    for T_, G in ((81, 1), (161, 2), (241, 3)):
        per = {k: len(ts) for k, ts in BD.static_deal(T_, G).items()}
        assert {k for k, c in per.items() if c == 6} == {(0, 0)} and set(per.values()) == {5, 6}
        assert BD.static_deal(T_, G)[(0, 0)] == list(range(0, T_, 16 * G))
        assert BD.static_deal(T_, G)[(G - 1, 15)][0] == 15 * G + G - 1 == 16 * G - 1
    # a split call of the 2-block size under grid 2: ten pieces of 16 tiles (15 full and 40 frames), on
    # ranges [0, 8) and [8, 16), and one of 5 tiles (277 frames) on [0, 2) and [2, 5)
    assert [(BD.tiles(m), m % 64) for _, m in BD.pieces(n2, GRID, BD.SPLIT)] == [(16, 40)] * 10 + [(5, 21)]
    assert BD.block_ranges(16, 2) == [(0, 8), (8, 16)] and BD.block_ranges(5, 2) == [(0, 2), (2, 5)]
    # the real grid, 4397 tiles on 256 blocks: every block owns 17 tiles, so one wave of each draws a
    # second tile, and these 45 own an 18th
    sizes = [b - a for a, b in BD.block_ranges(4397, 256)]
    assert set(sizes) == {17, 18}
    assert [b for b, s in enumerate(sizes) if s == 18] == [
        5, 11, 17, 22, 28, 34, 39, 45, 51, 56, 62, 68, 73, 79, 85, 91, 96, 102, 108, 113, 119, 125, 130, 136, 142, 147,
        153, 159, 164, 170, 176, 182, 187, 193, 199, 204, 210, 216, 221, 227, 233, 238, 244, 250, 255]
    assert sizes.count(18) == 4397 - 17 * 256 == 45
    # the direct kernel there: 4096 waves, a second round for the 301 whose first tile is below 301
    two = {k for k, ts in BD.static_deal(4397, 256).items() if len(ts) == 2}
    assert two == {(b, 0) for b in range(256)} | {(b, 1) for b in range(45)} and len(two) == 301
    assert all(len(ts) in (1, 2) for ts in BD.static_deal(4397, 256).values())
    # the tile-edge sizes at the real grid: one block per tile
    assert [BD.grid(n, GRID) for n in BD.EDGE_SIZES] == [1, 1, 1, 2, 2, 2, 3, 16, 16, 17]
    assert [BD.grid(n, GRID, 2) for n in BD.EDGE_SIZES] == [1, 1, 1, 2, 2, 2, 2, 2, 2, 2]


HOST_SRC = """#include "hfv_br_kernel.hip"
static_assert(hfv::kBrStageWaves == %d, "waves of a staged block");
static_assert(hfv::kBrWin == %d, "staged window, the least staged slot");
static_assert(hfv::kBrStageWaves * 64 == 1024, "the direct kernel's block has as many waves");
"""


def _host_parse(tmp_path, waves, win):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc builds this project; it parses the kernel file for the host here"
    src = tmp_path / ("consts_%d_%d.hip" % (waves, win))
    src.write_text(HOST_SRC % (waves, win))
    return subprocess.run([hipcc, "--offload-host-only", "-fsyntax-only", "-std=c++17", "-I", CSRC, str(src)],
                          capture_output=True, text=True)


def test_model_constants_are_the_kernels(tmp_path):
    """kBrStageWaves and kBrWin out of csrc/hfv_br_kernel.hip, through the compiler (host side only,
    no code generated): static assertions with the model's values hold, and fail with others."""
    r = _host_parse(tmp_path, BD.WAVES, BD.WIN)
    assert r.returncode == 0, r.stderr[-2000:]
    for waves, win in ((BD.WAVES - 1, BD.WIN), (BD.WAVES, BD.WIN * 2)):
        r = _host_parse(tmp_path, waves, win)
        assert r.returncode != 0 and "static assertion failed" in r.stderr, r.stderr[-2000:]
    src = open(os.path.join(CSRC, "hfv_br_kernel.hip")).read()
    # the launcher's arithmetic, as the model restates it
    assert "block = kBrStageWaves * 64;" in src and "block = 1024;" in src
    assert "tb0 = ntiles * blockIdx.x / gridDim.x" in src
    assert "__builtin_amdgcn_readfirstlane(wib) * gridDim.x + blockIdx.x" in src
    assert BD.SLOT % 16 == 0 and BD.SLOT >= BD.WIN and BD.DIRECT_SLOT % 16 == 8 and BD.DIRECT_SLOT % 8 == 0


# ---- the corpus ---------------------------------------------------------------------------------

def test_corpus_is_a_function_of_tile_and_lane():
    big = BD.corpus(BD.deal_size(3))
    for n in BD.EDGE_SIZES + (BD.deal_size(1),):
        assert all(np.array_equal(a, b[:n]) for a, b in zip(BD.corpus(n), big))
    frames, lens, ifidx = big
    k = BD.kinds(len(lens))
    (_, verdict, _, _), _ = BD.expected(len(lens))
    assert np.array_equal(verdict, np.array(BD.KIND_VERDICT)[k])        # every kind is what it is named
    for t in range(BD.tiles(len(lens)) - 1):                             # every full tile: all kinds, all odd ifindices
        sl = slice(64 * t, 64 * t + 64)
        assert set(k[sl]) == set(range(5)) and set(BD.ODD_IFINDEX) <= set(ifidx[sl].tolist())
        assert min(np.bincount(k[sl][:48], minlength=5)) >= 6
    assert len(np.unique(lens)) > 100 and len(np.unique(lens[k == 0])) >= 40   # lengths vary per frame
    assert (frames[:, 200:] != 0).all() and len(np.unique(frames[:, 200:], axis=0)) > 250   # the slot's rest is not blank


@pytest.mark.parametrize("n", SIZES)
def test_no_tile_can_stand_in_for_another(n):
    """Any two tiles of a run expect verdict vectors that differ in 8 lanes or more (a partial tile's
    missing lanes hold the GPU legs' pre-fill) and add different bytes to the byte counters."""
    _, lens, ifidx = BD.corpus(n)
    (_, verdict, _, _), _ = BD.expected(n)
    T_ = BD.tiles(n)
    v = np.full(T_ * 64, BD.FILL_VERDICT, np.uint8)
    v[:n] = verdict
    v = v.reshape(T_, 64)
    for lo in range(0, T_, 128):
        d = (v[lo:lo + 128, None, :] != v[None, :, :]).sum(axis=2)
        d[np.arange(len(d)), lo + np.arange(len(d))] = 64
        assert d.min() >= 8, (n, lo, d.min())
    tb = BD.tile_bytes(lens, ifidx, verdict)
    assert len(np.unique(tb, axis=0)) == T_ and (tb.sum(axis=1) > 0).all()


@pytest.mark.parametrize("hf_check", [True, False], ids=["hf_check", "hf_check_off"])
def test_no_tile_can_run_twice_or_not_at_all(hf_check):
    """Every full tile holds frames the router rewrites, a second run of the checker over its own
    output changes every full tile's frames or verdicts, and no expected output is the pre-fill."""
    frames, lens, ifidx = BD.corpus(REAL)
    (a, v, e, _), out = BD.expected(REAL, hf_check)
    again = out.copy()
    a2, v2, e2, _ = orc.br_process(again, lens, ifidx, T.br_config("br1"), BD.HK, hf_check=hf_check)
    full = REAL // 64
    per_tile = lambda x: x[:full * 64].reshape(full, -1).any(axis=1)   # noqa: E731
    assert per_tile((out != frames).any(axis=1)).all()
    assert per_tile((again != out).any(axis=1) | (v2 != v) | (a2 != a) | (e2 != e)).all()
    assert per_tile((v2 != v)).all()                     # the output elements alone show a second run
    assert not (a == BD.FILL_ACTION).any() and not (v == BD.FILL_VERDICT).any() and not (e == BD.FILL_EGRESS).any()
    assert BD.FILL_ACTION != 2 and BD.FILL_VERDICT != 0 and BD.FILL_EGRESS != -1       # nor a detached router's
    assert (v == BD.V["INVALID_HF"]).any() == hf_check
    gf, gl, gi = BD.guard_frames(68)
    ga, gv, _, _ = orc.br_process(gf.copy(), gl, gi, T.br_config("br1"), BD.HK, hf_check=hf_check)
    assert (gv == BD.V["SCION_FORWARD"]).all()           # a guard slot run by mistake is rewritten


def test_checker_against_the_reference_program_and_the_fixture():
    """The 5157-frame corpus: the checker's results equal tests/golden/br_deal.npz, what the reference
    program gave for it, and the reference program itself where it is built."""
    frames, lens, ifidx = BD.corpus(BD.deal_size(1))
    res, out = BD.expected(len(lens))
    g = orc.load_golden("br_deal.npz")
    assert g["sha256"].tobytes() == S.sha256(frames, lens, ifidx), "the generator drifted"
    orc.assert_br_equal(res, out, (g["action"], g["verdict"], g["egress"], g["stats"]), frames ^ g["xor"],
                        "checker against the fixture")
    if orc.ref_br_available():
        prog = frames.copy()
        orc.assert_br_equal(res, out, orc.ref_br_process(prog, lens, ifidx, T.br_config("br1"), BD.HK), prog,
                            "checker against the reference program")
