"""The tile dealing of k_br_process -- the staged kernel's block ranges and claimed tiles with the next
tile fetched ahead, the direct kernel's and the detached loop's static deal over several rounds, the
partial last tile, the split of a counting call -- on the sizes and the corpus of tests/br_deal.py,
against the CPU checker's results (held once per size against the reference program where it is built;
tests/test_br_deal.py holds them against tests/golden/br_deal.npz).  Integer work: every comparison is
bit-exact and covers every byte of every slot, action, verdict, egress and the counters.

Every buffer is larger than the call.  Four slots before frame 0 and 64 after frame n - 1 hold
forwardable frames (a wave that runs one rewrites it), with their lengths and ifindices beside them;
action, verdict and egress carry 64 elements on either side and are pre-filled with values no result
takes; the counters lie between two guard words; a 264-byte slot's spare bytes and the 16 bytes
around the frame buffer carry a fill.  All of it is compared afterwards.

Where a wave must run several tiles the launch is capped at 1, 2 or 3 blocks with the test build's
hfv_debug_br_grid, and a counting call is cut into pieces with hfv_debug_br_split, so those tests run in
a child process on lib/libscionhfv_test.so (conftest.rerun_on_test_build).  There every call also
asserts the kernel it meant to run (hfv_debug_br_last_variant).  The real-grid tests need no hook.

A mutant build (make brdeal) already has the hooks: run it with
HFV_LIB=lib/libscionhfv_brdealN.so HFV_TEST_BUILD_CHILD=1, which runs every test body in place.

Out of scope: launch_br_process' separate output buffer (reachable only through hfv_loop_run;
tests/test_gpu_loop.py holds it at one block), the automatic split of a counting call and the 32-bit
block counters near 2^32 bytes (gigabytes of frames per block)."""
import numpy as np
import pytest

import br_deal as BD
import br_topo as T
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build
from test_gpu_br import _ref_judges

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                        # output elements, lengths and ifindices on either side of the call
PRE_SLOTS, POST_SLOTS = 4, 64     # frame slots before frame 0 and after frame n - 1
GUARD_WORD = 0x5A5A5A5A5A5A5A5A
FILL_SPARE = 0xA5
NSTATS = hfv.BR_STATS_IFINDEX * 2 * hfv.BR_COUNTERS
CFG = T.br_config("br1")
_JUDGED = set()


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()
    if hasattr(hfv.lib(), "hfv_debug_br_grid"):   # (the parent process runs on the product library)
        hfv.Ctx.debug_br_grid(0)
        hfv.Ctx.debug_br_split(0)


def judged(n, hf_check=True):
    """BD.expected, held once against the reference program where it is built."""
    res, out = BD.expected(n, hf_check)
    if (n, hf_check) not in _JUDGED and _ref_judges(CFG, hf_check):
        frames, lens, ifidx = BD.corpus(n)
        prog = frames.copy()
        orc.assert_br_equal(res, out, orc.ref_br_process(prog, lens, ifidx, CFG, BD.HK, hf_check=hf_check), prog,
                            "checker against the reference program, n=%d" % n)
    _JUDGED.add((n, hf_check))
    return res, out


def real_n():
    return BD.real_size(torch.cuda.get_device_properties(0).multi_processor_count)


def setup_router(ctx, hf_check=True):
    ctx.br_set_build_options(0)
    ctx.br_set_config(CFG)
    ctx.br_set_hf_check(hf_check)
    ctx.key_add(0, T.KEYS[1])


class Call:
    """One hfv_br_process call over corpus(n) inside guarded device buffers.  form: "staged" (slot 256,
    aligned), "slot264" (slot % 16 != 0) or "offset8" (slot 256, frames 8 bytes off 16-byte alignment)."""

    def __init__(self, n, form, counted=True):
        self.n, self.form, self.counted = n, form, counted
        self.slot = slot = BD.DIRECT_SLOT if form == "slot264" else BD.SLOT
        off = 8 if form == "offset8" else 0
        frames, lens, ifidx = BD.corpus(n)
        gf, gl, gi = BD.guard_frames(PRE_SLOTS + POST_SLOTS)
        rows = np.full((PRE_SLOTS + n + POST_SLOTS, slot), FILL_SPARE, np.uint8)
        rows[:PRE_SLOTS, :BD.SLOT], rows[PRE_SLOTS + n:, :BD.SLOT] = gf[:PRE_SLOTS], gf[PRE_SLOTS:]
        rows[PRE_SLOTS:PRE_SLOTS + n, :BD.SLOT] = frames
        self.rows = rows
        self.base = torch.full((rows.size + 16,), FILL_SPARE, dtype=torch.uint8, device=DEV)
        assert self.base.data_ptr() % 16 == 0
        self.buf = self.base[off:off + rows.size]
        self.buf.copy_(torch.from_numpy(rows.reshape(-1)))
        self.pkts = self.buf[PRE_SLOTS * slot:]
        assert self.pkts.data_ptr() % 16 == off
        pre = np.arange(GUARD) % PRE_SLOTS          # before the call: forwardable lengths and ifindices too
        dl = np.concatenate([gl[pre], lens, gl[PRE_SLOTS:]])
        di = np.concatenate([gi[pre], ifidx, gi[PRE_SLOTS:]])
        self.dl = torch.from_numpy(dl.view(np.int16)).to(DEV)
        self.di = torch.from_numpy(di.view(np.int32)).to(DEV)
        m = GUARD + n + GUARD
        self.a = torch.full((m,), BD.FILL_ACTION, dtype=torch.uint8, device=DEV)
        self.v = torch.full((m,), BD.FILL_VERDICT, dtype=torch.uint8, device=DEV)
        self.e = torch.full((m,), BD.FILL_EGRESS, dtype=torch.int32, device=DEV)
        s = np.zeros(NSTATS + 2, np.uint64)
        s[0] = s[-1] = GUARD_WORD
        self.s = torch.from_numpy(s.view(np.int64)).to(DEV)

    def launch(self, ctx):
        g = GUARD
        ctx.br_process(self.pkts, self.slot, self.dl[g:], self.di[g:], self.n, self.a[g:], self.v[g:], self.e[g:],
                       self.s[1:] if self.counted else None)
        torch.cuda.synchronize()
        if hasattr(hfv.lib(), "hfv_debug_br_last_variant"):
            assert hfv.Ctx.debug_br_last_variant() == ("staged" if self.form == "staged" else "direct"), self.form

    def check(self, want, want_frames, what):
        """want: (action, verdict, egress, stats) of the n frames; want_frames u8[n, 256]."""
        n, g = self.n, GUARD
        what = "%s, n=%d, %s%s" % (what, n, self.form, "" if self.counted else ", no counters")
        a, v, e = self.a.cpu().numpy(), self.v.cpu().numpy(), self.e.cpu().numpy()
        s = self.s.cpu().numpy().view(np.uint64)
        got = self.buf.cpu().numpy().reshape(-1, self.slot)
        expect = self.rows.copy()
        expect[PRE_SLOTS:PRE_SLOTS + n, :BD.SLOT] = want_frames
        stats = s[1:-1] if self.counted else np.asarray(want[3]).reshape(-1)
        orc.assert_br_equal((a[g:g + n], v[g:g + n], e[g:g + n], stats), got[PRE_SLOTS:PRE_SLOTS + n],
                            want, expect[PRE_SLOTS:PRE_SLOTS + n], what)
        for name, x, fill in (("action", a, BD.FILL_ACTION), ("verdict", v, BD.FILL_VERDICT), ("egress", e, BD.FILL_EGRESS)):
            bad = np.nonzero(np.concatenate([x[:g], x[g + n:]]) != fill)[0]
            assert not len(bad), "%s: %s written outside the call, element %d" % (what, name, bad[0] - g if bad[0] < g else n + bad[0] - g)
        assert (got[:PRE_SLOTS] == expect[:PRE_SLOTS]).all(), what + ": a slot before frame 0 written"
        bad = np.nonzero((got[PRE_SLOTS + n:] != expect[PRE_SLOTS + n:]).any(axis=1))[0]
        assert not len(bad), "%s: slot n + %d written" % (what, bad[0])
        assert s[0] == GUARD_WORD and s[-1] == GUARD_WORD, what + ": a word beside the counters written"
        if not self.counted:
            assert not s[1:-1].any(), what + ": counters written by a call without counters"
        off = self.buf.data_ptr() - self.base.data_ptr()
        assert (self.base[:off] == FILL_SPARE).all() and (self.base[off + self.rows.size:] == FILL_SPARE).all(), what

    def check_detached(self, what):
        """Every frame passed up the stack, nothing else touched, nothing counted."""
        n = self.n
        want = (np.full(n, 2, np.uint8), np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.zeros(NSTATS, np.uint64))
        self.check(want, self.rows[PRE_SLOTS:PRE_SLOTS + n, :BD.SLOT], what + ", detached")


def run(ctx, n, form, cap=0, split=0, counted=True, hf_check=True, what=""):
    """One call against the checker.  cap, split: the test build's hooks (0: not touched)."""
    want, out = judged(n, hf_check)
    if cap or split:
        hfv.Ctx.debug_br_grid(cap)
        hfv.Ctx.debug_br_split(split)
    c = Call(n, form, counted)
    setup_router(ctx, hf_check)
    c.launch(ctx)
    c.check(want, out, "%sgrid %s%s%s" % (what, cap or "real", ", split %d" % split if split else "",
                                        "" if hf_check else ", hf check off"))


# ---- tile-edge sizes ----------------------------------------------------------------------------

@pytest.mark.parametrize("form", BD.FORMS)
def test_edge_sizes_real_grid(ctx, form):
    """n = 1, 63, 64, 65, ... 1025 on one block per tile: the partial last tile's write-back through a
    64-frame range, the fetch past the last tile, lanes past n."""
    for n in BD.EDGE_SIZES:
        run(ctx, n, form)


@pytest.mark.parametrize("form", BD.FORMS)
def test_edge_sizes_capped(request, ctx, form):
    """The same sizes on 1 and 2 blocks: 1024 frames are one round of one block, 1025 one tile more."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    for cap in (1, 2):
        for n in BD.EDGE_SIZES:
            run(ctx, n, form, cap=cap)


# ---- dealing sizes ------------------------------------------------------------------------------

@pytest.mark.parametrize("form", BD.FORMS)
def test_dealing_sizes(request, ctx, form):
    """64 * 16 * B * 5 + 37 frames on B = 1, 2, 3 blocks, five tiles per wave on average, with and
    without counters (the STATS = false kernels)."""
    if rerun_on_test_build(request):
        return
    for B in BD.CAPS:
        for counted in (True, False):
            run(ctx, BD.deal_size(B), form, cap=B, counted=counted)


def test_dealing_hf_check_off(request, ctx):
    """The hop-field check switched off: the bad-MAC frames are forwarded, on 2 staged blocks."""
    if rerun_on_test_build(request):
        return
    run(ctx, BD.deal_size(2), "staged", cap=2, hf_check=False)


@pytest.mark.parametrize("form", BD.FORMS)
def test_dealing_split(request, ctx, form):
    """A counting call in pieces of 1000 frames (no tile multiple) on 2 blocks: every piece dealt on
    its own, the counters added up."""
    if rerun_on_test_build(request):
        return
    run(ctx, BD.deal_size(2), form, cap=2, split=BD.SPLIT)


# ---- the real grid ------------------------------------------------------------------------------

@pytest.mark.parametrize("counted", [True, False], ids=["counters", "no_counters"])
@pytest.mark.parametrize("form", ["staged", "slot264"])
def test_real_grid(ctx, form, counted):
    """64 * (16 CUs + 300) + 37 frames on one block per CU: staged blocks of 17 and 18 tiles, a second
    round for part of the direct kernel's waves."""
    run(ctx, real_n(), form, counted=counted)


# ---- a detached router --------------------------------------------------------------------------

def test_detached_router(request, ctx, tmp_path, monkeypatch):
    """A pinned table marked detached: every frame gets action 2, verdict 0, egress -1, frames, guards
    and counters stay as they were -- on 1 and 3 blocks and on the real grid, by either kernel's loop.
    Republished, the same router routes again."""
    if rerun_on_test_build(request):
        return
    monkeypatch.setenv("HFV_PIN_DIR", str(tmp_path))
    path = hfv.brconfig_path("br1-ff00_0_1-1")
    hfv.brconfig_publish(path, CFG)
    ctx.br_set_build_options(0)
    ctx.br_set_config(hfv.BrConfig())
    ctx.br_set_hf_check(True)
    ctx.key_add(0, T.KEYS[1])
    ctx.attach_brconfig(path)
    for n, cap in ((BD.deal_size(1), 1), (BD.deal_size(3), 3), (real_n(), 0)):
        hfv.Ctx.debug_br_grid(cap)
        want, out = judged(n)
        for form in ("staged", "slot264"):
            hfv.brconfig_detach(path)
            c = Call(n, form)
            c.launch(ctx)
            c.check_detached("grid %s" % (cap or "real"))
            hfv.brconfig_publish(path, CFG)
            c = Call(n, form)
            c.launch(ctx)
            c.check(want, out, "republished, grid %s" % (cap or "real"))


# ---- which kernel ran ---------------------------------------------------------------------------

def test_variant_selection(request, ctx):
    """hfv_debug_br_last_variant follows the selection rule of launch_br_process."""
    if rerun_on_test_build(request):
        return
    setup_router(ctx)
    for form, want in (("staged", "staged"), ("slot264", "direct"), ("offset8", "direct"), ("staged", "staged")):
        c = Call(65, form)
        c.launch(ctx)
        assert hfv.Ctx.debug_br_last_variant() == want
