"""hfv_verify_frames_batches without a GPU: the two entry points are declared, exported by the
product and the test library and wrapped in Python; the ABI version stays 3; FrameBatch mirrors
struct hfv_frame_batch; a NULL ctx, a NULL list with count > 0 and a NULL kernel_ms are -EINVAL
before any device work; and the launch split and tile dealing restated in plain Python
(tests/frames_list.py) give every tile of every list to exactly one claim, with the batches placed
against the block ranges as the table below says."""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import frames_list as FL
import fused_deal as FD
import orc
import scion_hfv as hfv

NAMES = ("hfv_verify_frames_batches", "hfv_verify_frames_batches_timed")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_entry_points_declared_and_exported():
    src = open(os.path.join(orc.ROOT, "include", "scion_hfv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), name
    assert re.search(r"^struct\s+hfv_frame_batch\s*\{", src, flags=re.M)
    assert re.search(r"#define\s+HFV_ABI_VERSION\s+3\b", src)
    for path in (hfv.LIB_PATH, hfv.TEST_LIB_PATH):
        assert set(NAMES) <= _exports(path), path
    assert hfv.lib().hfv_abi_version() == 3


def test_python_wrappers():
    for name in ("verify_frames_batches", "verify_frames_batches_timed"):
        sig = inspect.signature(getattr(hfv.Ctx, name))
        assert list(sig.parameters) == ["self", "batches", "stream"]
        assert sig.parameters["stream"].default is None
    L = hfv.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert L.hfv_verify_frames_batches.argtypes == [vp, vp, sz, vp]
    assert L.hfv_verify_frames_batches_timed.argtypes == [vp, vp, sz, vp, ctypes.POINTER(ctypes.c_float)]


def test_frame_batch_layout():
    assert ctypes.sizeof(hfv.FrameBatch) == 56
    offsets = [(name, getattr(hfv.FrameBatch, name).offset) for name, _ in hfv.FrameBatch._fields_]
    assert offsets == [("frames", 0), ("slot", 8), ("len", 16), ("ingress_ifindex", 24), ("n", 32), ("status", 40),
                       ("pass_bits", 48)]
    # tuples: (frames, slot, lens, n, pass_bits[, ingress_ifindex[, status]])
    arr = hfv.Ctx.frame_batches([(0x1000, 256, 0x2000, 7, 0x3000), (0x10, 64, 0x20, 1, 0x30, 0x40, 0x50),
                                 hfv.FrameBatch(1, 2, 3, 4, 5, 6, 7)])
    got = [tuple(getattr(b, name) for name, _ in hfv.FrameBatch._fields_) for b in arr]
    assert got == [(0x1000, 256, 0x2000, None, 7, None, 0x3000), (0x10, 64, 0x20, 0x40, 1, 0x50, 0x30),
                   (1, 2, 3, 4, 5, 6, 7)]


def test_rejects_bad_arguments_without_gpu():
    """A NULL ctx, a NULL list with count > 0 and, in the timed form, a NULL kernel_ms fail with
    -EINVAL before any device work."""
    L = hfv.lib()
    E = -errno.EINVAL
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    arr = hfv.Ctx.frame_batches([(p, 64, p, 1, p)])
    ms = ctypes.c_float(-1.0)
    assert L.hfv_verify_frames_batches(None, arr, 1, None) == E
    assert "NULL" in L.hfv_last_error().decode()
    assert L.hfv_verify_frames_batches(None, None, 0, None) == E            # even with count == 0
    assert L.hfv_verify_frames_batches_timed(None, arr, 1, None, ctypes.byref(ms)) == E
    assert L.hfv_verify_frames_batches_timed(None, arr, 1, None, None) == E
    assert "null" in L.hfv_last_error().decode()
    assert ms.value == -1.0                                                  # nothing written on the failed call
    # the list is looked at before the device is: a NULL list with count > 0 needs no GPU to fail,
    # whatever the ctx pointer (it is not dereferenced before the list check)
    fake = ctypes.create_string_buffer(1 << 16)
    assert L.hfv_verify_frames_batches(ctypes.addressof(fake), None, 3, None) == E
    assert "null batch list" in L.hfv_last_error().decode()
    assert L.hfv_verify_frames_batches_timed(ctypes.addressof(fake), None, 3, None, ctypes.byref(ms)) == E
    assert ms.value == 0.0


# ---- the model -----------------------------------------------------------------------------------

# list -> keysel -> (launches, a block range starts mid-batch, most batches one forward step passes)
# on 1, 2, 3 and 256 blocks
PLACEMENT = {
    "ragged": {0: ((1, False, 5), (1, True, 5), (1, True, 5), (1, True, 0)),
               1: ((1, False, 5), (1, True, 5), (1, True, 5), (1, True, 0))},
    "empties": {0: ((1, False, 2), (1, True, 0), (1, True, 0), (1, True, 0)),
                1: ((1, False, 2), (1, True, 0), (1, True, 0), (1, True, 0))},
    "split33": {0: ((2, False, 11), (2, True, 11), (2, False, 0), (2, False, 0)),
                1: ((2, False, 9), (2, True, 9), (2, False, 9), (2, True, 0))},
    "split70": {0: ((3, False, 11), (3, True, 11), (3, True, 0), (3, True, 0)),
                1: ((3, False, 9), (3, True, 9), (3, True, 9), (3, True, 0))},
    "mixed": {0: ((6, False, 5), (6, True, 0), (6, True, 0), (6, True, 0)),
              1: ((6, False, 4), (6, True, 0), (6, True, 0), (6, True, 0))},
    "direction": {0: ((1, False, 2), (1, True, 2), (1, True, 2), (1, True, 0)),
                  1: ((1, False, 2), (1, True, 1), (1, True, 2), (1, True, 0))},
}
# the dealing lists (kind, keysel) on the grid they are made for: 1, 2, 3 and 256 blocks
DEAL_PLACEMENT = {
    ("small", 0): ((1, False, 4), (1, True, 5), (1, True, 5), (4, True, 0)),
    ("large", 0): ((1, False, 3), (1, True, 2), (1, True, 1), (1, True, 2)),
    ("small", 1): ((1, False, 3), (1, True, 3), (1, True, 4), (4, True, 0)),
    ("large", 1): ((1, False, 3), (1, True, 2), (1, True, 1), (1, True, 2)),
}


def cap_of(grid):
    return 0 if grid == FD.REAL_GRID else grid


def deal_specs(kind, keysel, grid):
    return [FL.Spec(FL.FUZZ[0], 0, n, FL.DEAL_SLOT) for n in FL.deal_sizes(kind, keysel, grid)]


def all_lists():
    for name in FL.LISTS:
        for keysel in FL.KEYSELS:
            for grid in FL.GRIDS:
                yield (name, keysel, grid), FL.specs(name), keysel, cap_of(grid)
    for kind in ("small", "large"):
        for keysel in FL.KEYSELS:
            for grid in FL.GRIDS:
                yield (kind, keysel, grid), deal_specs(kind, keysel, grid), keysel, cap_of(grid)


def test_launch_split():
    """Launches keep list order, hold 1..32 non-empty batches that are all staged or all direct,
    and end only at 32 batches or at a change of stageability."""
    for what, specs, _, _ in all_lists():
        ls, flags = FL.launches(specs)
        flat = [i for launch in ls for i, _ in launch]
        assert flat == [i for i, s in enumerate(specs) if s.n], what
        for launch, staged in zip(ls, flags):
            assert 1 <= len(launch) <= FL.BATCH_MAX
            assert all(FL.stageable(specs[i].slot, specs[i].shift) == staged for i, _ in launch), what
        for a, b, fa, fb in zip(ls, ls[1:], flags, flags[1:]):
            assert len(a) == FL.BATCH_MAX or fa != fb, what
    assert FL.launches([FL.EMPTY] * 3) == ([], []) and FL.launches([]) == ([], [])
    ls, flags = FL.launches(FL.specs("mixed"))
    assert flags == [True, False, True, False, True, False]


def test_every_tile_maps_to_one_batch_tile_and_is_claimed_once():
    for what, specs, keysel, cap in all_lists():
        ls, flags = FL.launches(specs)
        for launch, staged in zip(ls, flags):
            d = FL.deal(launch, staged, keysel, cap)
            assert 1 <= d.G <= (cap or FD.REAL_GRID) and d.G <= max(1, -(-d.T // FD.WAVES[keysel])), what
            assert d.ranges[0][0] == 0 and d.ranges[-1][1] == d.T
            assert all(a[1] == b[0] for a, b in zip(d.ranges, d.ranges[1:]))
            assert all(hi > lo for lo, hi in d.ranges), (what, "a block without a tile")
            # the map is a bijection between global tiles and (batch, tile) pairs, nf in 1..64
            want = {(j, t) for j, n in enumerate(d.n) for t in range(FD.tiles_of(n))}
            got = [FL.tile_of(d, g) for g in range(d.T)]
            assert len(got) == len(want) and {x[:2] for x in got} == want, what
            assert all(1 <= nf <= 64 for _, _, nf in got)
            assert all(sum(nf for j, _, nf in got if j == k) == n for k, n in enumerate(d.n))
            seen = FL.owners(d, keysel)
            assert set(seen) == want and set(seen.values()) == {1}, what


def test_placement_table():
    for name, by_keysel in PLACEMENT.items():
        for keysel, row in by_keysel.items():
            got = tuple(tuple(FL.placement(FL.specs(name), keysel, cap_of(g))) for g in FL.GRIDS)
            assert got == row, (name, keysel, got)
    for (kind, keysel), row in DEAL_PLACEMENT.items():
        got = tuple(tuple(FL.placement(deal_specs(kind, keysel, g), keysel, cap_of(g))) for g in FL.GRIDS)
        assert got == row, (kind, keysel, got)
    # what the GPU tests rely on: on two blocks every list has a block range that starts inside a
    # batch; on one block a forward step passes two batches or more in every list; the split lists
    # make two and three launches, the mixed one a launch per change of staging
    assert all(PLACEMENT[name][k][1][1] for name in PLACEMENT for k in FL.KEYSELS)
    assert all(PLACEMENT[name][k][0][2] >= 2 for name in PLACEMENT for k in FL.KEYSELS)
    assert [PLACEMENT[n][0][0][0] for n in ("split33", "split70", "mixed")] == [2, 3, 6]
    assert all(DEAL_PLACEMENT[(kind, k)][3][1] for kind in ("small", "large") for k in FL.KEYSELS)
    assert all(DEAL_PLACEMENT[("large", k)][3][2] >= 2 for k in FL.KEYSELS)


def test_list_shapes():
    assert [s.n for s in FL.specs("ragged")] == list(FL.RAGGED_N)
    assert [s.n == 0 for s in FL.specs("empties")] == [True, False, True, True, False, False, True]
    for name, count in (("split33", 33), ("split70", 70)):
        assert len(FL.specs(name)) == count and all(1 <= s.n <= 130 for s in FL.specs(name))
    m = FL.specs("mixed")
    assert {s.slot for s in m} == set(FL.SLOTS_STAGED + FL.SLOTS_DIRECT) and any(s.shift == 8 for s in m)
    for slot in (256, 136):      # the whole corpus of a BR in either kind of launch
        assert sum(s.n for s in m if s.src == ("corpus", "br1", False) and s.slot == slot) == 1188
    d = FL.specs("direction")
    assert {(s.ifx > 0, s.status) for s in d} == {(a, b) for a in (False, True) for b in (False, True)}
    assert d[0]._replace(ifx=1) == d[1] and d[0]._replace(ifx=2) == d[4]
    assert all(sum(s.n for s in FL.specs(name)) <= 20000 for name in FL.LISTS)


@pytest.mark.parametrize("name", list(FL.LISTS))
def test_lists_hold_both_verdicts(name):
    """Each list holds at least 100 passing and 100 failing frames, every batch of 256 frames or more
    at least one of each, and (so that a vote past n shows) every fuzz batch wider than slot 64
    ends on a passing frame."""
    for keysel in FL.KEYSELS:
        npass = nfail = 0
        for s in FL.specs(name):
            if not s.n:
                continue
            words, st = FL.expected(s, keysel)
            p = FL.passes_of(words, s.n)
            assert len(words) == FD.tiles_of(s.n) and len(st) == s.n
            assert not (p & (st != 0)).any()
            npass, nfail = npass + int(p.sum()), nfail + int((~p).sum())
            if s.n >= 256:
                assert p.any() and not p.all(), (name, s)
            if keysel == 0 and s.src[0] == "fuzz" and s.slot > 64:
                assert p[-1], (name, s)
        assert npass >= 100 and nfail >= 100, (name, keysel, npass, nfail)


def test_direction_matters():
    """The same frames under NULL, their own and another ifindex array give three different bitmaps."""
    d = FL.specs("direction")
    w = [FL.expected(d[i], 0)[0] for i in (0, 1, 4)]
    bits = [FL.passes_of(x, d[0].n) for x in w]
    assert (bits[0] != bits[1]).sum() >= 100 and (bits[1] != bits[2]).sum() >= 100 and (bits[0] != bits[2]).sum() >= 100
    # and the statuses do not depend on it
    assert all(np.array_equal(FL.expected(d[0], 0)[1], FL.expected(d[i], 0)[1]) for i in (1, 4))


def test_dealing_lists():
    """TILES_PER_WAVE tiles per wave and more on the capped grids and in the large list; no full
    tile's word is 0, all ones or the bitmap's fill."""
    for keysel in FL.KEYSELS:
        _, _, passes = FL.deal_case(keysel)
        assert 500 < passes.sum() < FL.CYCLE - 500
        for kind in ("small", "large"):
            for grid in FL.GRIDS:
                sizes = FL.deal_sizes(kind, keysel, grid)
                tiles = sum(FD.tiles_of(n) for n in sizes)
                if kind == "large" or grid != FD.REAL_GRID:
                    assert tiles >= FL.TILES_PER_WAVE * FD.WAVES[keysel] * grid
                assert any(n % 64 for n in sizes)
        words = FL.deal_words(passes, 0, 64 * FL.CYCLE)
        assert not (words == 0).any() and not (words == np.uint64(2**64 - 1)).any()
        assert not (words == np.uint64(0xC3A5C3A5C3A5C3A5)).any()
