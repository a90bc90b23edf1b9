"""The window-edge corpus of tests/br_shift.py on the GPU: forwardable frames whose PathMeta,
SegIDs, hop field and MAC lie in front of, across and past bytes 128 and 136 (the end of the
staged row and of the router's ext registers), through every kernel that reads frame headers
through a window: hfv_br_process staged and unstaged, hfv_br_process_host at every window,
hfv_loop_run, hfv_extract_records[_rx] and hfv_verify_frames.  Bit-exact against the oracle
router / the host parser, the oracle held against the reference program where it is built and
against tests/golden/br_shift.npz everywhere.

`make winedge` builds libraries with one wrong window-edge case each; this module must fail on
every one of them (HFV_LIB=lib/libscionhfv_winedgeN.so) except the one no frame can tell from the
product (N = 2, see hfv_br_kernel.hip)."""
import numpy as np
import pytest

import br_fuzz as F
import br_shift as S
import br_topo as T
import frames_rx_ref as R
import orc
import scion_hfv as hfv
from test_gpu_br import _ref_judges
from test_gpu_frames import reslot
from test_gpu_frames_rx import check_extract_rx, run_extract_rx, run_verify_frames_rx
from test_gpu_loop import _oracle as loop_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = hfv.VERDICT
HK = orc.hop_key(T.KEYS[1])
FAMILIES = pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
FORMS = ("staged", "slot264", "offset8")
GUARD = 5            # rows and output entries past n, filled and compared
FILL_FRAME, FILL_OUT = 0xA5, 0x5A


@pytest.fixture()
def fctx():
    """A fresh ctx for the frame kernels: default record layout and keysel, no keys, empty set."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()


def setup_router(ctx, cfg):
    ctx.br_set_build_options(0)
    ctx.br_set_config(cfg)
    ctx.br_set_hf_check(True)
    ctx.key_add(0, T.KEYS[1])


def run_router(ctx, cfg, frames, lens, ifidx, form):
    """hfv_br_process over frames[n, 256] in a device buffer of n + GUARD rows: slot 256 (the
    staged kernel), slot 264 (slot % 16 != 0: the kernel without staging) or slot 256 from a
    buffer 8 bytes off 16-byte alignment (unstaged by alignment).  Rows past n, the 8 spare bytes
    of a 264-byte slot and the outputs past n carry a fill.  Returns ((action, verdict, egress)
    of n + GUARD entries, stats, the whole buffer [n + GUARD, slot], the buffer as it went in)."""
    n = len(frames)
    slot = 264 if form == "slot264" else 256
    off = 8 if form == "offset8" else 0
    rows = np.full((n + GUARD, slot), FILL_FRAME, np.uint8)
    rows[:n, :frames.shape[1]] = frames
    base = torch.full(((n + GUARD) * slot + 16,), FILL_FRAME, dtype=torch.uint8, device=DEV)
    assert base.data_ptr() % 16 == 0
    d = base[off:off + (n + GUARD) * slot]
    d.copy_(torch.from_numpy(rows.reshape(-1)))
    dl = torch.from_numpy(np.concatenate([lens, np.zeros(GUARD, np.uint16)]).view(np.int16)).to(DEV)
    di = torch.from_numpy(np.concatenate([ifidx, np.zeros(GUARD, np.uint32)]).view(np.int32)).to(DEV)
    a = torch.full((n + GUARD,), FILL_OUT, dtype=torch.uint8, device=DEV)
    v = torch.full((n + GUARD,), FILL_OUT, dtype=torch.uint8, device=DEV)
    e = torch.full((n + GUARD,), -77, dtype=torch.int32, device=DEV)
    s = torch.zeros(hfv.BR_STATS_IFINDEX * 2 * hfv.BR_COUNTERS, dtype=torch.int64, device=DEV)
    setup_router(ctx, cfg)
    ctx.br_process(d, slot, dl, di, n, a, v, e, s)
    torch.cuda.synchronize()
    assert (base[:off] == FILL_FRAME).all() and (base[off + (n + GUARD) * slot:] == FILL_FRAME).all()
    stats = s.cpu().numpy().view(np.uint64).reshape(orc.BR_STATS_SHAPE)
    return (a.cpu().numpy(), v.cpu().numpy(), e.cpu().numpy()), stats, d.cpu().numpy().reshape(n + GUARD, slot), rows


def check_router(ctx, cfg, frames, lens, ifidx, form, want, want_frames, what):
    """One form against (action, verdict, egress, stats) and the expected frames [n, 256]."""
    n = len(frames)
    (a, v, e), stats, got, rows = run_router(ctx, cfg, frames, lens, ifidx, form)
    expect = rows.copy()
    expect[:n, :frames.shape[1]] = want_frames
    orc.assert_br_equal((a[:n], v[:n], e[:n], stats), got[:n], want, expect[:n], "%s, %s" % (what, form))
    assert (got[n:] == FILL_FRAME).all(), "rows past n written"
    assert (a[n:] == FILL_OUT).all() and (v[n:] == FILL_OUT).all() and (e[n:] == -77).all(), "outputs past n written"


_JUDGED = set()


def judged_oracle(name, br, v6, frames, lens, ifidx):
    """The oracle's results on a fixture leg, held once against the reference program where it is
    built (the leg of test_gpu_br._compare)."""
    res, out = S.oracle(name)
    cfg = T.br_config(br, v6)
    if name not in _JUDGED and _ref_judges(cfg):
        prog = frames.copy()
        orc.assert_br_equal(res, out, orc.ref_br_process(prog, lens, ifidx, cfg, HK), prog,
                            "oracle against the reference program, " + name)
    _JUDGED.add(name)
    return res, out


# ---- hfv_br_process -----------------------------------------------------------------------------

@FAMILIES
@pytest.mark.parametrize("br", S.BRS)
@pytest.mark.parametrize("form", FORMS)
def test_router_corpus(gpu_ctx, form, br, v6):
    frames, lens, ifidx, _, _ = S.shift_corpus(v6)[br]
    res, out = judged_oracle(S.corpus_name(br, v6), br, v6, frames, lens, ifidx)
    assert (res[1] == V["SCION_FORWARD"]).all()
    check_router(gpu_ctx, T.br_config(br, v6), frames, lens, ifidx, form, res, out, "corpus %s" % br)


@FAMILIES
@pytest.mark.parametrize("form", FORMS[:2])
def test_router_truncation_sweep(gpu_ctx, form, v6):
    frames, lens, ifidx = S.truncation_sweep(v6)
    res, out = judged_oracle(S.sweep_name(v6), "br1", v6, frames, lens, ifidx)
    check_router(gpu_ctx, T.br_config("br1", v6), frames, lens, ifidx, form, res, out, "sweep")


def test_router_against_the_fixture(gpu_ctx):
    """The staged kernel against tests/golden/br_shift.npz alone: what the reference program gave
    for the corpus and the sweep.  Needs no reference build."""
    g = orc.load_golden("br_shift.npz")
    for name, br, v6, frames, lens, ifidx in S.fixture_legs():
        assert g[name + "_sha256"].tobytes() == S.sha256(frames, lens, ifidx), "the generator drifted: " + name
        want = (g[name + "_action"], g[name + "_verdict"], g[name + "_egress"], g[name + "_stats"])
        check_router(gpu_ctx, T.br_config(br, v6), frames, lens, ifidx, "staged", want, frames ^ g[name + "_xor"], name)


@FAMILIES
@pytest.mark.parametrize("order", ["interleaved", "permuted"])
def test_router_tile_mixing(gpu_ctx, order, v6):
    """The br1 corpus interleaved frame by frame with as many fuzz frames (parse failures, bad
    MACs, truncations, other interfaces), so the lanes of one wave take different window cases in
    the same instruction; once in that order and once under a fixed permutation."""
    cf, cl, ci, _, _ = S.shift_corpus(v6)["br1"]
    n = len(cf)
    ff, fl, fi = F.fuzz_batch(S.hop_inputs(v6), "br1", v6, n, seed=41 + v6, slot=S.SLOT)
    frames = np.empty((2 * n, S.SLOT), np.uint8)
    lens, ifidx = np.empty(2 * n, np.uint16), np.empty(2 * n, np.uint32)
    frames[0::2], lens[0::2], ifidx[0::2] = cf, cl, ci
    frames[1::2], lens[1::2], ifidx[1::2] = ff, fl, fi
    if order == "permuted":
        p = np.random.default_rng(7).permutation(2 * n)
        frames, lens, ifidx = np.ascontiguousarray(frames[p]), lens[p], ifidx[p]
    cfg = T.br_config("br1", v6)
    out = frames.copy()
    res = orc.br_process(out, lens, ifidx, cfg, HK)
    if _ref_judges(cfg):
        prog = frames.copy()
        orc.assert_br_equal(res, out, orc.ref_br_process(prog, lens, ifidx, cfg, HK), prog, "oracle against the reference")
    assert (res[1] == V["SCION_FORWARD"]).sum() >= n and len(np.unique(res[1])) >= 5
    check_router(gpu_ctx, cfg, frames, lens, ifidx, "staged", res, out, "tile mixing")


# ---- hfv_br_process_host ------------------------------------------------------------------------

def check_host_path(ctx, v6, frames, lens, ifidx, want, want_frames, window, register=False, cfg=None):
    n = len(frames)
    setup_router(ctx, T.br_config("br1", v6) if cfg is None else cfg)
    got = hfv.host_array(frames.shape, np.uint8) if register else np.empty_like(frames)
    got[:] = frames
    a, v, e = np.full(n, FILL_OUT, np.uint8), np.full(n, FILL_OUT, np.uint8), np.full(n, -77, np.int32)
    st = np.zeros(orc.BR_STATS_SHAPE, np.uint64)
    if register:
        ctx.host_register(got)
    try:
        ctx.br_process_host(got, frames.shape[1], lens, ifidx, n, a, v, e, st, window=window)
    finally:
        if register:
            ctx.host_unregister(got)
    # the counters too: a frame re-run whole because its headers pass the window counts once
    orc.assert_br_equal((a, v, e, st), got, want, want_frames, "host path, window %d" % window)


HOST_WINDOWS = S.HOST_WINDOWS_ALL_ABOVE + S.HOST_WINDOWS + (256,)


@FAMILIES
@pytest.mark.parametrize("window", HOST_WINDOWS + ("zerocopy",))
def test_host_path_corpus(gpu_ctx, window, v6):
    """Pageable frames at every header window (104, 120, 136 and 152 are no multiple of 16 and
    112 is below 128: the kernel without staging; 128, 144, 160 and 256 the staged one), and once
    registered (zero-copy)."""
    frames, lens, ifidx, _, _ = S.shift_corpus(v6)["br1"]
    res, out = S.oracle(S.corpus_name("br1", v6))
    if window == "zerocopy":
        check_host_path(gpu_ctx, v6, frames, lens, ifidx, res, out, 0, register=True)
    else:
        check_host_path(gpu_ctx, v6, frames, lens, ifidx, res, out, window)


@FAMILIES
@pytest.mark.parametrize("window", [120, 128])
def test_host_path_truncation_sweep(gpu_ctx, window, v6):
    frames, lens, ifidx = S.truncation_sweep(v6)
    res, out = S.oracle(S.sweep_name(v6))
    check_host_path(gpu_ctx, v6, frames, lens, ifidx, res, out, window)


# ---- hfv_loop_run -------------------------------------------------------------------------------

@pytest.mark.parametrize("slot", [256, 240])
@pytest.mark.parametrize("dma", [0, 1, 2], ids=["zero_copy", "dma", "dma_in_zc_out"])
def test_loop_corpus(gpu_ctx, dma, slot):
    """The br1 IPv4 corpus through the loop, one run per ingress interface (the loop takes one
    ifindex per run); in 240-byte ring slots the frames sit at other addresses than in the corpus'
    own 256-byte rows.  Counts, verdict histogram and the digest of every transmitted frame."""
    frames, lens, ifidx, _, _ = S.shift_corpus(False)["br1"]
    assert lens.max() <= 240
    cfg = T.br_config("br1")
    for ifx in sorted(set(ifidx.tolist())):
        sel = np.nonzero(ifidx == ifx)[0]
        rows, ln = np.ascontiguousarray(frames[sel][:, :slot]), lens[sel]
        total = len(sel) + 37
        setup_router(gpu_ctx, cfg)
        got = gpu_ctx.loop_run(rows, ln, total, rx_ifindex=int(ifx), slot=slot, chunk=100, chunks=3, producers=2,
                               consumers=2, digest=True, dma=dma)
        want = loop_oracle(rows, total, True, lens=ln, cfg=cfg, key=T.KEYS[1], rx_ifindex=int(ifx), slot=slot)
        assert want["tx"] == total and want["drop"] == 0
        for k in want:
            assert got[k] == want[k], (k, ifx)


# ---- hfv_extract_records / _rx, hfv_verify_frames -----------------------------------------------

_EXTRACT = {}


def frame_legs(v6, slot):
    """[(name, frames [n, slot], lens, ifindex, internal set)]: the corpus per BR and the sweep."""
    if (v6, slot) not in _EXTRACT:
        legs = []
        for name, br, fam, frames, lens, ifidx in S.fixture_legs():
            if fam == v6:
                legs.append((name, reslot(frames, slot), lens, ifidx, R.internal_ifindices(T.br_config(br, v6))))
        _EXTRACT[(v6, slot)] = legs
    return _EXTRACT[(v6, slot)]


@FAMILIES
@pytest.mark.parametrize("layout", [(40, 48, 64), (0, 8, 24)], ids=lambda x: "-".join(map(str, x)))
@pytest.mark.parametrize("slot", [256, 136], ids=["staged", "direct"])
def test_extract_corpus_and_sweep(fctx, slot, layout, v6):
    """hfv_extract_records and hfv_extract_records_rx (the BR's internal interfaces as the set)
    against hfv_frame_extract per frame: status, info and hop field, frames unwritten, records and
    status past n untouched.  In 136-byte slots the longer frames are cut by the slot."""
    inf_off, hf_off, stride = layout
    parsed = 0
    for name, frames, lens, ifidx, iset in frame_legs(v6, slot):
        n = len(frames)
        st, _, _ = check_extract_rx(fctx, frames, lens, ifidx, iset, n, layout)
        fctx.set_internal_ifindices([])
        got_st, recs = run_extract_rx(fctx, frames, lens, None, n, layout, rx=False)
        want_st, inf, hf = R.frame_extract(frames, lens, False)
        assert np.array_equal(want_st, st)
        assert np.array_equal(got_st[:n], want_st), name
        assert np.array_equal(recs[:n, inf_off:inf_off + 8], inf) and np.array_equal(recs[:n, hf_off:hf_off + 12], hf), name
        assert (got_st[n:] == 0xA5).all() and (recs[n:] == 0xA5).all(), "wrote past n"
        if name.startswith("corpus") and slot == 256:
            assert (st == 0).all()
        parsed += int((st == 0).sum())
    assert parsed >= (400 if slot == 256 else 100)


@FAMILIES
def test_verify_frames_corpus_vs_router_oracle(fctx, v6):
    """hfv_verify_frames on the br1 corpus and on a copy with one MAC bit flipped per frame: for
    the frames from an external interface the pass bit is the router oracle's SCION_FORWARD."""
    frames, lens, ifidx, _, _ = S.shift_corpus(v6)["br1"]
    bad = frames.copy()
    for i in range(len(bad)):
        bad[i, S.field_offsets(bytes(frames[i]))["mac"][0] + i % 6] ^= 1 << (i % 8)
    frames, lens, ifidx = np.concatenate([frames, bad]), np.concatenate([lens, lens]), np.concatenate([ifidx, ifidx])
    cfg = T.br_config("br1", v6)
    _, verdict, _, _ = orc.br_process(frames.copy(), lens, ifidx, cfg, HK)
    sel = ~np.isin(ifidx, R.internal_ifindices(cfg)) & np.isin(verdict, [V["SCION_FORWARD"], V["INVALID_HF"]])
    n = len(frames)
    assert sel.sum() >= n // 3 and (verdict[sel] == V["INVALID_HF"]).sum() == sel.sum() // 2
    fctx.key_add(0, T.KEYS[1])
    got, st = run_verify_frames_rx(fctx, frames, lens, ifidx, n, rx=False)
    assert (st == 0).all()
    assert np.array_equal(hfv.bits_to_bool(got, n)[sel], verdict[sel] == V["SCION_FORWARD"])
