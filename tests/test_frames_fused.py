"""hfv_verify_frames_fused without a GPU: the two entry points are declared, exported by the product
and the test library and wrapped in Python; the ABI version stays 3; a NULL ctx or a NULL kernel_ms
is -EINVAL before any device work; and the kernel's tile dealing, restated in plain Python
(tests/fused_deal.py), gives every tile of every size the GPU tests run to exactly one claim."""
import ctypes
import errno
import inspect
import os
import re
import subprocess

import pytest

import fused_deal as FD
import orc
import scion_hfv as hfv

NAMES = ("hfv_verify_frames_fused", "hfv_verify_frames_fused_timed")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_entry_points_declared_and_exported():
    src = open(os.path.join(orc.ROOT, "include", "scion_hfv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), name
    assert re.search(r"#define\s+HFV_ABI_VERSION\s+3\b", src)
    for path in (hfv.LIB_PATH, hfv.TEST_LIB_PATH):
        assert set(NAMES) <= _exports(path), path
    assert hfv.lib().hfv_abi_version() == 3


def test_python_wrappers():
    for name in ("verify_frames_fused", "verify_frames_fused_timed"):
        params = list(inspect.signature(getattr(hfv.Ctx, name)).parameters)
        assert params == ["self", "frames", "slot", "lens", "n", "pass_bits", "ingress_ifindex", "status", "stream"]
        sig = inspect.signature(getattr(hfv.Ctx, name))
        assert all(sig.parameters[p].default is None for p in ("ingress_ifindex", "status", "stream"))


def test_rejects_bad_arguments_without_gpu():
    """A NULL ctx, and a NULL kernel_ms in the timed form, fail with -EINVAL before any device work,
    whatever the other arguments are."""
    L = hfv.lib()
    E = -errno.EINVAL
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    ms = ctypes.c_float(-1.0)
    assert L.hfv_verify_frames_fused(None, p, 64, p, None, 1, None, p, None) == E
    assert "NULL" in L.hfv_last_error().decode()
    assert L.hfv_verify_frames_fused(None, None, 64, None, None, 0, None, None, None) == E     # even with n == 0
    assert L.hfv_verify_frames_fused_timed(None, p, 64, p, None, 1, None, p, None, ctypes.byref(ms)) == E
    assert L.hfv_verify_frames_fused_timed(None, p, 64, p, None, 1, None, p, None, None) == E
    assert "null" in L.hfv_last_error().decode()
    assert ms.value == -1.0                                   # nothing written on the failed call


@pytest.mark.parametrize("keysel", [0, 1], ids=["zero", "ifid"])
def test_block_ranges_and_claims_cover_every_tile_once(keysel):
    """1, 2, 3 and 256 blocks over every size the GPU tests use: the block ranges tile [0, T), the
    claims of a block's waves walk its range in order, and no tile is claimed twice or never."""
    for cap in FD.CAPS + (0,):
        sizes = FD.TEST_SIZES + tuple(FD.deal_n(keysel, b) for b in FD.CAPS + (FD.REAL_GRID,))
        for n in sizes:
            T, G = FD.tiles_of(n), FD.grid(n, keysel, cap=cap)
            assert 1 <= G <= (cap or FD.REAL_GRID) and G <= max(1, -(-T // FD.WAVES[keysel]))
            edges = [FD.block_range(T, G, k) for k in range(G)]
            assert edges[0][0] == 0 and edges[-1][1] == T
            assert all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
            assert all(hi > lo for lo, hi in edges), "a block without a tile"
            for k, (lo, hi) in enumerate(edges):
                taken, _ = FD.claims(T, G, k, FD.WAVES[keysel])
                assert taken == list(range(lo, hi))
            assert FD.owners(n, keysel, cap=cap) == [1] * T, (n, cap)


@pytest.mark.parametrize("keysel", [0, 1], ids=["zero", "ifid"])
def test_dealing_sizes_give_every_wave_five_tiles(keysel):
    for b in FD.CAPS + (FD.REAL_GRID,):
        n = FD.deal_n(keysel, b)
        T, G = FD.tiles_of(n), FD.grid(n, keysel, cap=0 if b == FD.REAL_GRID else b)
        assert G == b and n % 64 == 37
        per_block = [hi - lo for lo, hi in (FD.block_range(T, G, k) for k in range(G))]
        assert min(per_block) >= FD.TILES_PER_WAVE * FD.WAVES[keysel]
        assert b == 1 or len(set(per_block)) > 1, "the block ranges are not ragged"
