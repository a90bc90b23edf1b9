"""The SCION path walk on the GPU -- parse_scion_path, as_ingress, as_egress, the info field step after
a segment switch, the PathMeta and SegID stores of rewrite, and keep_mac_bytes / mac_b8 / clob, which
make the deferred MAC check see the bytes from before the rewrite -- on the corpus of tests/br_walk.py,
against the CPU checker's results (held once per leg against the reference program where it is built,
and against tests/golden/br_walk.npz), and frame_locate of the frame kernels on the same frames against
the host parser.  Integer work: every comparison is bit-exact and covers every byte of every slot,
action, verdict, egress and the counters.

The corpus runs in two orders, since a wave runs each branch of the walk once for all its lanes:
shuffled (every 64-frame tile mixes kinds) and sorted (whole tiles on one branch); by the staged kernel
and by the direct one (a slot that is no multiple of 16, or frames 8 bytes off 16-byte alignment); on
the real grid and, on the test build, on one block.  A few forwardable frames lie before and behind the
call and are compared too.

A mutant build (make pathwalk) already has the hooks: run it with
HFV_LIB=lib/libscionhfv_pathwalkN.so HFV_TEST_BUILD_CHILD=1, which runs every test body in place."""
import numpy as np
import pytest

import br_walk as W
import frames_rx_ref as R
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build
from test_gpu_br import _ref_judges

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = hfv.VERDICT
FAMILIES = [False, True]
FAM_IDS = ["ipv4", "ipv6"]
FORMS = ("staged", "slot1032", "offset8")
GUARD_SLOTS = 4
FILL_SPARE, FILL_OUT, FILL_EGRESS = 0xA5, 0x5A, -77
NSTATS = hfv.BR_STATS_IFINDEX * 2 * hfv.BR_COUNTERS
_JUDGED = set()


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()
    if hasattr(hfv.lib(), "hfv_debug_br_grid"):
        hfv.Ctx.debug_br_grid(0)


def judged(v6, hf_check=True, key=True):
    """W.expected, held once against the reference program where it is built."""
    res, out = W.expected(v6, hf_check, key)
    c = W.corpus(v6)
    if (v6, hf_check, key) not in _JUDGED and key and _ref_judges(c.cfg, hf_check):
        prog = c.frames.copy()
        orc.assert_br_equal(res, out, orc.ref_br_process(prog, c.lens, c.ifidx, c.cfg, W.HK, hf_check=hf_check), prog,
                            "checker against the reference program")
    _JUDGED.add((v6, hf_check, key))
    return res, out


def setup_router(ctx, v6, hf_check=True, key=True):
    ctx.br_set_build_options(0)
    ctx.br_set_config(W.corpus(v6).cfg)
    ctx.br_set_hf_check(hf_check)
    if key:
        ctx.key_add(0, W.KEY)


def guard_frames(v6):
    """GUARD_SLOTS forwardable frames (a wave that runs one rewrites it) with lengths and ifindices."""
    c = W.corpus(v6)
    (_, verdict, _, _), _ = W.expected(v6)
    k = np.nonzero((verdict == V["SCION_FORWARD"]) & (c.kind == "base"))[0][:GUARD_SLOTS]
    return c.frames[k], c.lens[k], c.ifidx[k]


def run_br(ctx, v6, order, form, counted=True, hf_check=True, key=True, cap=0, want=None):
    """One hfv_br_process call over the corpus in the given order, against the checker (or `want`)."""
    c = W.corpus(v6)
    (wa, wv, we, ws), wout = want or judged(v6, hf_check, key)
    perm = W.orders(v6)[order]
    n, g = c.n, GUARD_SLOTS
    slot = 1032 if form == "slot1032" else W.SLOT
    off = 8 if form == "offset8" else 0
    gf, gl, gi = guard_frames(v6)
    rows = np.full((g + n + g, slot), FILL_SPARE, np.uint8)
    rows[:g, :W.SLOT], rows[g + n:, :W.SLOT] = gf, gf
    rows[g:g + n, :W.SLOT] = c.frames[perm]
    base = torch.full((rows.size + 16,), FILL_SPARE, dtype=torch.uint8, device=DEV)
    assert base.data_ptr() % 16 == 0
    buf = base[off:off + rows.size]
    buf.copy_(torch.from_numpy(rows.reshape(-1)))
    dl = torch.from_numpy(np.concatenate([gl, c.lens[perm], gl]).view(np.int16)).to(DEV)
    di = torch.from_numpy(np.concatenate([gi, c.ifidx[perm], gi]).view(np.int32)).to(DEV)
    a = torch.full((n + 2 * g,), FILL_OUT, dtype=torch.uint8, device=DEV)
    v = torch.full((n + 2 * g,), FILL_OUT, dtype=torch.uint8, device=DEV)
    e = torch.full((n + 2 * g,), FILL_EGRESS, dtype=torch.int32, device=DEV)
    s = torch.zeros(NSTATS + 2, dtype=torch.int64, device=DEV)
    if cap:
        hfv.Ctx.debug_br_grid(cap)
    setup_router(ctx, v6, hf_check, key)
    ctx.br_process(buf[g * slot:], slot, dl[g:], di[g:], n, a[g:], v[g:], e[g:], s[1:] if counted else None)
    torch.cuda.synchronize()
    if hasattr(hfv.lib(), "hfv_debug_br_last_variant"):
        assert hfv.Ctx.debug_br_last_variant() == ("staged" if form == "staged" else "direct"), form
    what = "%s, %s, %s%s%s%s%s" % ("ipv6" if v6 else "ipv4", order, form, "" if counted else ", no counters",
                                   "" if hf_check else ", hf check off", "" if key else ", no key", ", one block" if cap else "")
    ga, gv, ge, gs = a.cpu().numpy(), v.cpu().numpy(), e.cpu().numpy(), s.cpu().numpy().view(np.uint64)
    got = buf.cpu().numpy().reshape(-1, slot)
    expect = rows.copy()
    expect[g:g + n, :W.SLOT] = wout[perm]
    try:
        orc.assert_br_equal((ga[g:g + n], gv[g:g + n], ge[g:g + n], gs[1:-1] if counted else ws), got[g:g + n],
                            (wa[perm], wv[perm], we[perm], ws), expect[g:g + n], what)
    except AssertionError as err:                            # name the first frame by what it is
        bad = np.nonzero((gv[g:g + n] != wv[perm]) | (got[g:g + n] != expect[g:g + n]).any(axis=1))[0]
        it = c.items[perm[bad[0]]] if len(bad) else None
        raise AssertionError("%s; corpus frame %s" % (err, it and (int(perm[bad[0]]), it.kind, it.what, it.layout, it.ci, it.ch,
                                                                it.cons, it.direction, it.cut)))
    assert (ga[:g] == FILL_OUT).all() and (ga[g + n:] == FILL_OUT).all() and (gv[:g] == FILL_OUT).all(), what
    assert (gv[g + n:] == FILL_OUT).all() and (ge[:g] == FILL_EGRESS).all() and (ge[g + n:] == FILL_EGRESS).all(), what
    assert (got[:g] == expect[:g]).all() and (got[g + n:] == expect[g + n:]).all(), what + ": a slot beside the call written"
    assert gs[0] == 0 and gs[-1] == 0 and (counted or not gs.any()), what + ": counters"
    assert (base[:off] == FILL_SPARE).all() and (base[off + rows.size:] == FILL_SPARE).all(), what
    return gv[g:g + n], perm


# ---- hfv_br_process -----------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_br_process(ctx, v6, order, form):
    """Frames, action, verdict, egress and counters of the whole corpus, by the staged and the direct
    kernel, tiles of mixed kinds and tiles of one kind."""
    run_br(ctx, v6, order, form)


@pytest.mark.parametrize("form", ["staged", "slot1032"])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_br_process_without_counters(ctx, v6, form):
    run_br(ctx, v6, "shuffled", form, counted=False)


@pytest.mark.parametrize("form", ["staged", "slot1032"])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_br_process_hf_check_off(ctx, v6, form):
    """Every overlap frame, both kinds of twins included, is then forwarded."""
    gv, perm = run_br(ctx, v6, "shuffled", form, hf_check=False)
    c = W.corpus(v6)
    assert (gv[(c.kind == "overlap")[perm]] == V["SCION_FORWARD"]).all() and not (gv == V["INVALID_HF"]).any()


@pytest.mark.parametrize("form", ["staged", "slot1032"])
def test_br_process_without_a_key(ctx, form):
    """No key in slot 0: every frame that reaches the MAC check is INVALID_HF, rewritten all the same."""
    gv, _ = run_br(ctx, False, "sorted", form, key=False)
    assert (gv == V["INVALID_HF"]).sum() > 5000 and (gv == V["SCION_FORWARD"]).sum() > 500   # (between siblings: no check)


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_br_process_against_the_fixture(ctx, v6):
    """tests/golden/br_walk.npz: what the reference program gave, without the checker in between."""
    c = W.corpus(v6)
    g, fam = orc.load_golden("br_walk.npz"), "v6" if v6 else "v4"
    want = c.frames.copy()
    want[:, :W.FIXTURE_WIDTH] ^= g["xor_" + fam]
    gv, perm = run_br(ctx, v6, "shuffled", "staged",
                      want=((g["action_" + fam], g["verdict_" + fam], g["egress_" + fam], g["stats_" + fam]), want))
    over = (c.kind == "overlap")[perm]
    assert sorted(zip(c.what[perm][over].tolist(), gv[over].tolist())) == sorted(
        [("d0", 12)] * 2 + [("d0_after", 81)] * 2 + [("d4", 81)] * 3 + [("d8", 12)] + [("d8_after", 81)] * 2)


@pytest.mark.parametrize("form", ["staged", "slot1032"])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_br_process_on_one_block(request, ctx, v6, form):
    """hfv_debug_br_grid(1): every wave of one block runs tile after tile of the corpus, in both orders;
    the kernel that ran is asserted."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    for order in ("shuffled", "sorted"):
        run_br(ctx, v6, order, form, cap=1)


# ---- hfv_br_process_host ------------------------------------------------------------------------

@pytest.mark.parametrize("window", [0, 128, 256])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_br_process_host(ctx, v6, window):
    """Only the first `window` bytes of each slot go up: the frames whose hop field lies deeper are run
    again whole, with the same frames, results and counters."""
    c = W.corpus(v6)
    (wa, wv, we, ws), wout = judged(v6)
    perm = W.orders(v6)["shuffled"]
    setup_router(ctx, v6)
    got = np.ascontiguousarray(c.frames[perm])
    a, v = np.full(c.n, FILL_OUT, np.uint8), np.full(c.n, FILL_OUT, np.uint8)
    e = np.full(c.n, FILL_EGRESS, np.int32)
    st = np.zeros(orc.BR_STATS_SHAPE, np.uint64)
    ctx.br_process_host(got, W.SLOT, np.ascontiguousarray(c.lens[perm]), np.ascontiguousarray(c.ifidx[perm]), c.n, a, v, e,
                        st, window=window)
    orc.assert_br_equal((a, v, e, st), got, (wa[perm], wv[perm], we[perm], ws), wout[perm],
                        "host path, window %d, %s" % (window, "ipv6" if v6 else "ipv4"))
    hf = np.array([w.hf if w.hf is not None else 0 for w in (c.walk(i) for i in range(c.n))])
    assert ((hf + c.P + 12 > 256) & (wv == V["SCION_FORWARD"])).sum() > 1000    # forwarded from past every window


# ---- the frame kernels --------------------------------------------------------------------------

class Frames:
    """The corpus of one family on the device with what the frame kernels must give: status and the
    8 + 12 bytes by the host parser, the bits by the record checker on those records."""

    def __init__(self, v6):
        c = self.c = W.corpus(v6)
        self.n = c.n
        self.iset = R.internal_ifindices(c.cfg)
        self.st, self.inf, self.hf = R.frame_extract(c.frames, c.lens, c.internal)
        self.st_ext, self.inf_ext, self.hf_ext = R.frame_extract(c.frames, c.lens, False)
        hk, valid = orc.key_table(W.KEY)
        self.bits = R.oracle_bits(self.st, self.inf, self.hf, hk, valid, hfv.KEYSEL_ZERO)
        self.bits_ext = R.oracle_bits(self.st_ext, self.inf_ext, self.hf_ext, hk, valid, hfv.KEYSEL_ZERO)
        # the frames the hop-field MAC decides (frames_rx_ref.Batch selects them so)
        (_, verdict, _, _), _ = W.expected(v6)
        decided = np.isin(verdict, [V["SCION_FORWARD"], V["INVALID_HF"]])
        ext_ifid = sorted(k for k, (kind, _) in W.EGRESS.items() if kind == "link")
        _, inf0, hf0 = self.st_ext, self.inf_ext, self.hf_ext.astype(np.uint32)
        cons = (inf0[:, 0] & 1) == 1
        egr = np.where(cons, hf0[:, 4] << 8 | hf0[:, 5], hf0[:, 2] << 8 | hf0[:, 3])
        self.sel = decided & (~c.internal | np.isin(egr, ext_ifid))
        self.forward = verdict == V["SCION_FORWARD"]
        assert self.sel.sum() > 9000 and (self.forward & self.sel).sum() > 4000 and (~self.forward & self.sel).sum() > 4000
        self._dev = None

    def dev(self):
        """(frames, lens, ifindices) on the device."""
        if self._dev is None:
            c = self.c
            self._dev = (torch.from_numpy(c.frames.copy()).to(DEV), torch.from_numpy(c.lens.view(np.int16).copy()).to(DEV),
                         torch.from_numpy(c.ifidx.view(np.int32).copy()).to(DEV))
        return self._dev

    def check_records(self, st, recs, rx):
        want = (self.st, self.inf, self.hf) if rx else (self.st_ext, self.inf_ext, self.hf_ext)
        bad = np.nonzero((st != want[0]) | (recs[:, 0:8] != want[1]).any(axis=1) | (recs[:, 8:20] != want[2]).any(axis=1))[0]
        assert not len(bad), ("status or record", len(bad), bad[:4], [self.c.items[i].layout for i in bad[:4]])

    def check_bits(self, words, rx=True):
        assert np.array_equal(words, self.bits if rx else self.bits_ext), "bits against the record checker"
        if rx:
            b = hfv.bits_to_bool(words, self.n)
            assert np.array_equal(b[self.sel], self.forward[self.sel]), "bit against the router's verdict"
            over = {k: b[(self.c.kind == "overlap") & (self.c.what == k)].tolist() for k in W.OVERLAP}
            assert over == {"d8": [True], "d8_after": [False, False], "d0": [True, True], "d0_after": [False, False]}


_FRAMES = {}


def frames_of(v6):
    if v6 not in _FRAMES:
        _FRAMES[v6] = Frames(v6)
    return _FRAMES[v6]


def outs(n, fill=0xA5):
    return (torch.full((n, hfv.FRAME_REC_STRIDE), fill, dtype=torch.uint8, device=DEV),
            torch.full((n,), fill, dtype=torch.uint8, device=DEV),
            torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=DEV))


def words(bits):
    return bits.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_extract_records(ctx, v6):
    f = frames_of(v6)
    d, dl, di = f.dev()
    ctx.set_record_layout(0, 8)
    ctx.set_internal_ifindices(f.iset)
    for rx in (False, True):
        recs, st, _ = outs(f.n)
        if rx:
            ctx.extract_records_rx(d, W.SLOT, dl, di, f.n, recs, st)
        else:
            ctx.extract_records(d, W.SLOT, dl, f.n, recs, st)
        torch.cuda.synchronize()
        f.check_records(st.cpu().numpy(), recs.cpu().numpy(), rx)
    assert np.array_equal(d.cpu().numpy(), f.c.frames), "frames were written"


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_verify_frames_rx(ctx, v6):
    f = frames_of(v6)
    ctx.set_record_layout(0, 8)
    ctx.set_internal_ifindices(f.iset)
    ctx.key_add(0, W.KEY)
    recs, st, bits = outs(f.n)
    d, dl, di = f.dev()
    ctx.verify_frames_rx(d, W.SLOT, dl, di, f.n, recs, st, bits)
    torch.cuda.synchronize()
    f.check_records(st.cpu().numpy(), recs.cpu().numpy(), True)
    f.check_bits(words(bits))


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_verify_frames_fused(ctx, v6):
    f = frames_of(v6)
    ctx.set_internal_ifindices(f.iset)
    ctx.key_add(0, W.KEY)
    _, st, bits = outs(f.n)
    d, dl, di = f.dev()
    ctx.verify_frames_fused(d, W.SLOT, dl, f.n, bits, ingress_ifindex=di, status=st)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), f.st)
    f.check_bits(words(bits))
    _, st, bits = outs(f.n)
    ctx.verify_frames_fused(d, W.SLOT, dl, f.n, bits, status=st)           # no ifindices: every frame external
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), f.st_ext)
    f.check_bits(words(bits), rx=False)


@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_verify_frames_batches(ctx, v6):
    """One list cut from the corpus at tile multiples: ragged batches, an empty one among them."""
    f = frames_of(v6)
    ctx.set_internal_ifindices(f.iset)
    ctx.key_add(0, W.KEY)
    cuts = [0, 64, 64, 64 * 7, 64 * 100, 64 * 101, f.n // 64 * 64, f.n]
    _, st, bits = outs(f.n)
    d, dl, di = f.dev()
    ctx.verify_frames_batches([(d[a:], W.SLOT, dl[a:], b - a, bits[a // 64:], di[a:], st[a:]) for a, b in zip(cuts, cuts[1:])])
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), f.st)
    f.check_bits(words(bits))


@pytest.mark.parametrize("window", [0, 128])
@pytest.mark.parametrize("v6", FAMILIES, ids=FAM_IDS)
def test_verify_frames_host(ctx, v6, window):
    f = frames_of(v6)
    ctx.set_internal_ifindices(f.iset)
    ctx.key_add(0, W.KEY)
    bits = np.full((f.n + 63) // 64, 2**64 - 1, np.uint64)
    st = np.full(f.n, 0xA5, np.uint8)
    retried = ctx.verify_frames_host(np.ascontiguousarray(f.c.frames), W.SLOT, np.ascontiguousarray(f.c.lens), f.n, bits,
                                     ingress_ifindex=np.ascontiguousarray(f.c.ifidx), status=st, window=window)
    assert np.array_equal(st, f.st)
    f.check_bits(bits)
    assert retried > 1000                                    # the deep hop fields lie past either window
