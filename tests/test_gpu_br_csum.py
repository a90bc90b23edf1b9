"""The checksum-edge corpus of tests/br_csum.py on the GPU: forwardable frames whose checksum
residuals sit on every carry and sign edge of the reference's two-fold rule (D = 0, +-1, +-65535,
+-65536, multiples of 65535, bit 16 left after the second fold, wrapped sums whose result is 0x0000
or one off an ordinary update, incoming fields of 0x0000 and 0xffff), through hfv_br_process staged
and unstaged, hfv_br_process_host and hfv_loop_run.  Each table's frames are interleaved with
ordinary fuzz frames, so a tile holds forwarded and dropped frames.  Bit-exact against the oracle
router, the oracle held against the reference program where it is built and against
tests/golden/br_csum.npz everywhere.

`make csumedge` builds libraries with one wrong checksum rule each; this module must fail on every
one of them (HFV_LIB=lib/libscionhfv_csumedgeN.so)."""
import numpy as np
import pytest

import br_csum as C
import br_fuzz as F
import br_shift as S
import br_topo as T
import orc
from test_gpu_br import _ref_judges
from test_gpu_br_shift import FORMS, check_host_path, check_router, setup_router
from test_gpu_loop import _oracle as loop_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HK = orc.hop_key(T.KEYS[1])
LEGS = ("v4_base", "v4_mid", "v4_hi", "v4_lo", "v6_base", "v6_hi", "v6_lo")
_MIXED = {}


def mixed(name):
    """(cfg, v6, frames, lens, ifindex, oracle results, oracle frames, corpus rows) of leg `name`: its
    corpus frames at the even rows, as many fuzz frames of br1 (32 at least) in between and behind.
    The oracle runs once, and once against the reference program where it is built."""
    if name not in _MIXED:
        _, v6, table, cfg, cf, cl, ci, _ = next(leg for leg in C.legs() if leg[0] == name)
        n = len(cf)
        m = max(n, 32)
        ff, fl, fi = F.fuzz_batch(S.hop_inputs(v6), "br1", v6, m, seed=61 + LEGS.index(name), slot=C.SLOT)
        rows = np.arange(n) * 2
        rest = np.setdiff1d(np.arange(n + m), rows)
        frames = np.empty((n + m, C.SLOT), np.uint8)
        lens, ifidx = np.empty(n + m, np.uint16), np.empty(n + m, np.uint32)
        frames[rows], lens[rows], ifidx[rows] = cf, cl, ci
        frames[rest], lens[rest], ifidx[rest] = ff, fl, fi
        out = frames.copy()
        res = orc.br_process(out, lens, ifidx, cfg, HK)
        if _ref_judges(cfg):
            prog = frames.copy()
            orc.assert_br_equal(res, out, orc.ref_br_process(prog, lens, ifidx, cfg, HK), prog,
                                "oracle against the reference program, " + name)
        assert (res[1][rows] == C.FORWARD).all() and (res[1][rest] != C.FORWARD).any()
        assert np.array_equal(out[rows], C.oracle(name)[1])
        _MIXED[name] = (cfg, v6, frames, lens, ifidx, res, out, rows)
    return _MIXED[name]


@pytest.mark.parametrize("name", LEGS)
@pytest.mark.parametrize("form", FORMS)
def test_router_corpus(gpu_ctx, form, name):
    """hfv_br_process staged, at slot 264 and 8 bytes off alignment, with guard rows and fills."""
    cfg, v6, frames, lens, ifidx, res, out, _ = mixed(name)
    check_router(gpu_ctx, cfg, frames, lens, ifidx, form, res, out, "checksum edges, " + name)


def test_router_against_the_fixture(gpu_ctx):
    """The staged kernel against tests/golden/br_csum.npz alone: the fixture's frames and tables and
    what the reference program gave for them.  Needs no reference build."""
    for name, cfg, frames, lens, ifidx, want, want_frames in C.fixture_legs(orc.load_golden("br_csum.npz")):
        check_router(gpu_ctx, cfg, frames, lens, ifidx, "staged", want, want_frames, name)


@pytest.mark.parametrize("name", LEGS)
@pytest.mark.parametrize("mode", ["window", "zerocopy"])
def test_host_path_corpus(gpu_ctx, mode, name):
    """hfv_br_process_host at the default header window (pageable frames) and registered."""
    cfg, v6, frames, lens, ifidx, res, out, _ = mixed(name)
    check_host_path(gpu_ctx, v6, frames, lens, ifidx, res, out, 0, register=mode == "zerocopy", cfg=cfg)


@pytest.mark.parametrize("name", LEGS)
def test_loop_corpus(gpu_ctx, name):
    """The corpus frames of each table through the loop (copies both ways), one run per ingress
    interface: counts, verdict histogram and the digest of every transmitted frame."""
    _, v6, table, cfg, frames, lens, ifidx, _ = next(leg for leg in C.legs() if leg[0] == name)
    for ifx in sorted(set(ifidx.tolist())):
        sel = np.nonzero(ifidx == ifx)[0]
        rows, ln = np.ascontiguousarray(frames[sel]), lens[sel]
        total = len(sel) + 37
        setup_router(gpu_ctx, cfg)
        got = gpu_ctx.loop_run(rows, ln, total, rx_ifindex=int(ifx), slot=C.SLOT, chunk=100, chunks=3, producers=2,
                               consumers=2, digest=True, dma=1)
        want = loop_oracle(rows, total, True, lens=ln, cfg=cfg, key=T.KEYS[1], rx_ifindex=int(ifx), slot=C.SLOT)
        assert want["tx"] == total and want["drop"] == 0
        for k in want:
            assert got[k] == want[k], (k, name, ifx)
