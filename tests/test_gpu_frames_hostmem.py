"""hfv_verify_frames_host on the GPU: frames in host memory in, verdict bits out.

Every case has two judges.  The first is hfv_verify_frames_fused on a device copy of the full slots,
compared bit for bit, status too (the call's contract).  The second, for the corpus cases, is
independent of every kernel: hfv_frame_extract per frame on the host with the record checker
orc.verify_records (frames_hostmem.oracle, the judge of test_gpu_frames_fused.py).  The number of
frames run again must equal the count of the rule restated in tests/frames_hostmem.py, exactly; on the
zero-copy path it is 0.

Every bitmap and status array is pre-filled with garbage and guarded on both sides, and the frames,
lengths and ifindices are compared unchanged afterwards.  Integer work: every comparison is exact.

The tests that set the chunk size or cap the grid use test hooks and run in a child process on
lib/libscionhfv_test.so (conftest.rerun_on_test_build).

`make hostwin` builds three libraries with one wrong step each (csrc/hfv_frames_fused_kernel.hip); this
module must fail on every one: run it with HFV_LIB=lib/libscionhfv_hostwinN.so HFV_TEST_BUILD_CHILD=1.
The call runs on the two-slot schedule of csrc/hfv_host_pipe.h, so on lib/libscionhfv_hostchunk1.so
(`make hostchunk`: a retired chunk's results go to the other slot's place) both cases of
test_chunks_of_128 must fail as well, by an assertion or the call's own -EIO, never by a fault."""
import ctypes
import errno

import numpy as np
import pytest

import br_topo as T
import frames_hostmem as H
import frames_rx_ref as R
import host_chunks as HC
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BITS_FILL = 0xC3A5C3A5C3A5C3A5     # neither 0 nor all-ones: a word never stored cannot pass for a verdict word
ST_FILL = 0x5A                     # no status value
GUARD = 64                         # status bytes on either side (a tile's worth), bitmap words: 1
K1 = T.KEYS[1]
SLOT = H.SLOT


def _require(name):
    assert hasattr(hfv.lib(), name), name + " is not exported by " + (hfv.os.environ.get("HFV_LIB") or hfv.LIB_PATH)


@pytest.fixture()
def ctx():
    _require("hfv_verify_frames_host")   # a library without the entry point fails every test here
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)                  # a fresh ctx: default keysel, no keys, empty set
    yield c
    c.synchronize()
    c.close()


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def key1():
    return cached("key1", lambda: orc.key_table(K1))


def ifid_raw():
    def make():
        raw = bytearray(orc.gen_key_table(256))
        for ifid in range(1, 7):
            raw[16 * ifid:16 * ifid + 16] = K1
        return bytes(raw)
    return cached("ifid_raw", make)


def iset1():
    return sorted(set(R.internal_ifindices(T.br_config("br1", False))) | set(R.internal_ifindices(T.br_config("br1", True))))


def reslot(frames, slot):
    out = np.zeros((len(frames), slot), dtype=np.uint8)
    w = min(slot, frames.shape[1])
    out[:, :w] = frames[:, :w]
    return out


def tail(n, slot=SLOT):
    """The last n frames of the corpus: the last one is a long-path frame that passes and is undecided
    at every window below its hop field."""
    frames, lens, ifidx, _ = H.corpus()
    return reslot(frames[-n:], slot), np.array(lens[-n:]), np.array(ifidx[-n:])


def npass(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def judge(ctx, frames, lens, n, ifidx):
    """hfv_verify_frames_fused on a device copy: (words, status)."""
    d = torch.from_numpy(np.array(frames[:n], copy=True)).to(DEV)
    dl = torch.from_numpy(np.ascontiguousarray(lens[:n], dtype=np.uint16).view(np.int16).copy()).to(DEV)
    di = None if ifidx is None else torch.from_numpy(
        np.ascontiguousarray(ifidx[:n], dtype=np.uint32).view(np.int32).copy()).to(DEV)
    bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device=DEV)
    st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ctx.verify_frames_fused(d, frames.shape[1], dl, n, bits, ingress_ifindex=di, status=st)
    torch.cuda.synchronize()
    return bits.cpu().numpy().view(np.uint64), st.cpu().numpy()


def run_host(ctx, frames, lens, n, ifidx, window, status=True, ring=None, outs=None):
    """The call over the first n frames, from exact-size copies of the inputs.  ring: a registered
    host array the frames are placed in (zero-copy); outs: (bitmap, status) arrays to use instead of
    fresh guarded ones.  Returns (words, status or None, retried)."""
    slot = frames.shape[1]
    src = np.array(frames[:n], copy=True)
    if ring is not None:
        ring[:n * slot] = src.reshape(-1)
        fr = ring[:n * slot]
    else:
        fr = src.reshape(-1).copy()
    ln = np.array(lens[:n], dtype=np.uint16, copy=True)
    ix = None if ifidx is None else np.array(ifidx[:n], dtype=np.uint32, copy=True)
    words = (n + 63) // 64
    if outs is None:
        bits = np.full(words + 2, BITS_FILL, np.uint64)
        st = np.full(n + 2 * GUARD, ST_FILL, np.uint8) if status else None
    else:
        bits, st = outs
        bits[:] = BITS_FILL
        st[:] = ST_FILL
    retried = ctx.verify_frames_host(fr, slot, ln, n, bits[1:1 + words], ingress_ifindex=ix,
                                     status=None if st is None else st[GUARD:GUARD + n], window=window)
    assert np.array_equal(fr.reshape(n, slot), src), "frames were written"
    assert np.array_equal(ln, lens[:n]) and (ix is None or np.array_equal(ix, ifidx[:n])), "inputs were written"
    assert bits[0] == np.uint64(BITS_FILL) and bits[words + 1] == np.uint64(BITS_FILL), "wrote outside the bitmap"
    got_st = None
    if st is not None:
        assert (st[:GUARD] == ST_FILL).all() and (st[GUARD + n:] == ST_FILL).all(), "wrote outside status"
        got_st = st[GUARD:GUARD + n].copy()
    return bits[1:1 + words].copy(), got_st, retried


def check(ctx, frames, lens, n, ifidx, window, want=None, what="", **kw):
    """One call against hfv_verify_frames_fused on the device copy (and `want`, an independent
    (words, status), where given); retried against the model.  Returns (words, status, retried)."""
    jw, js = judge(ctx, frames, lens, n, ifidx)
    got, got_st, retried = run_host(ctx, frames, lens, n, ifidx, window, **kw)
    print(what, "window", window, "n", n, "retried", retried, "pass", npass(got))
    if got_st is not None:
        assert np.array_equal(got_st, js), ("status", what, window, np.nonzero(got_st != js)[0][:8])
    bad = np.nonzero(got != jw)[0]
    assert not len(bad), (what, window, "%d bad words, first %d: got %016x want %016x" % (
        len(bad), bad[0], int(got[bad[0]]), int(jw[bad[0]])))
    if n % 64:
        assert int(got[-1]) >> (n % 64) == 0, "a bit at or past n is set"
    if want is not None:
        assert np.array_equal(got, want[0]) and (got_st is None or np.array_equal(got_st, want[1])), ("oracle", what)
    slot = frames.shape[1]
    model = 0 if kw.get("ring") is not None else int(H.retried(frames[:n], lens[:n], window or min(256, slot)).sum())
    assert retried == model, ("retried", what, window, retried, model)
    return got, got_st, retried


def corpus_want(keysel=hfv.KEYSEL_ZERO, keys=None, with_set=True, n=None):
    frames, lens, ifidx, _ = H.corpus()
    n = len(frames) if n is None else n
    keys = keys or (key1() if keysel == hfv.KEYSEL_ZERO else orc.key_table(ifid_raw()))
    internal = np.isin(ifidx, iset1()) if with_set else False
    return H.oracle(frames, lens, n, internal, keys[0], keys[1], keysel)


# ---- the corpus at every window ----------------------------------------------------------------

@pytest.mark.parametrize("window", H.WINDOWS + (SLOT,))
def test_corpus_pageable(ctx, window):
    frames, lens, ifidx, _ = H.corpus()
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    want = cached("want0", corpus_want)
    got, st, retried = check(ctx, frames, lens, len(frames), ifidx, window, want=want, what="corpus")
    assert 100 < npass(got) < (st == 0).sum()                 # both verdicts among the parsed frames
    for s in (0, 17, 26, 34):
        assert (st == s).any(), s
    assert (retried == 0) == (window == SLOT)


@pytest.mark.parametrize("registered_outs", [False, True], ids=["outs-copied", "outs-in-place"])
def test_zero_copy_ring(ctx, registered_outs):
    frames, lens, ifidx, _ = H.corpus()
    n = len(frames)
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    ring = hfv.host_array(n * SLOT, np.uint8)
    outs, regs = None, [ring]
    if registered_outs:
        outs = (hfv.host_array((n + 63) // 64 + 2, np.uint64), hfv.host_array(n + 2 * GUARD, np.uint8))
        regs += list(outs)
    for r in regs:
        ctx.host_register(r)
    try:
        _, _, retried = check(ctx, frames, lens, n, ifidx, 128, want=cached("want0", corpus_want), what="zero-copy",
                              ring=ring, outs=outs)
        assert retried == 0
        check(ctx, frames, lens, n - 3, None, 0, what="zero-copy, no ifindex, no status", ring=ring, status=False)
    finally:
        for r in regs:
            ctx.host_unregister(r)


# ---- counts, chunks, alignment, slots ----------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_counts(ctx, n):
    """The last frame passes and is run again: its bit is the last one set, and a lane past n that
    voted with the clamped frame would mark a frame that does not exist."""
    frames, lens, ifidx = tail(n)
    ctx.key_add(0, K1)
    got, st, retried = check(ctx, frames, lens, n, ifidx, 128, what="counts")
    assert (int(got[-1]) >> ((n - 1) % 64)) & 1 == 1 and st[-1] == 0 and retried >= 1


@pytest.mark.parametrize("n", [3 * 128 + 37, 2 * 128])
def test_chunks_of_128(request, ctx, n):
    """Several chunks on both streams, a partial last chunk, and at window 64 a second run of several
    bounce chunks."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    frames, lens, ifidx = tail(n)
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    try:
        hfv.Ctx.debug_frames_host_chunk(128)
        def counts_hold(retried):
            got = hfv.Ctx.debug_host_chunk_counts()
            model = HC.counts(n, 128)
            assert (got[0], got[3]) == (model[0], model[3]) and got[2] == retried, ("counts", got, model, retried)

        for window in (64, 128, 256):
            _, _, retried = check(ctx, frames, lens, n, ifidx, window, what="chunk 128")
            counts_hold(retried)
            assert window != 64 or retried > 128              # two bounce chunks or more
        _, _, retried = check(ctx, frames, lens, n, None, 128, what="chunk 128, no status", status=False)
        counts_hold(retried)
    finally:
        hfv.Ctx.debug_frames_host_chunk(0)
    assert hfv.lib().hfv_debug_frames_host_chunk(ctypes.c_size_t(100)) == -errno.EINVAL   # not a multiple of 64


def test_frames_at_odd_alignment(ctx):
    frames, lens, ifidx = tail(300)
    n = 300
    ctx.key_add(0, K1)
    jw, js = judge(ctx, frames, lens, n, ifidx)
    buf = np.zeros(n * SLOT + 16, np.uint8)
    off = 1 + (-buf.ctypes.data) % 16                          # 1 past a 16-byte boundary
    view = buf[off:off + n * SLOT]
    view[:] = frames.reshape(-1)
    bits = np.full((n + 63) // 64, BITS_FILL, np.uint64)
    st = np.full(n, ST_FILL, np.uint8)
    assert view.ctypes.data % 16 == 1
    retried = ctx.verify_frames_host(view, SLOT, lens, n, bits, ingress_ifindex=ifidx, status=st, window=128)
    assert np.array_equal(bits, jw) and np.array_equal(st, js)
    assert retried == H.retried(frames, lens, 128).sum() and np.array_equal(view, frames.reshape(-1))


@pytest.mark.parametrize("slot", [256, 264, 1024])
def test_slots(ctx, slot):
    """264 is no multiple of 16: its whole-slot window and second run take the unstaged kernels.  In
    256- and 264-byte slots the long-path frames are cut by the slot."""
    frames, lens, ifidx, _ = H.corpus()
    fr = reslot(frames, slot)
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    for window in (0, 128, slot):
        got, _, _ = check(ctx, fr, lens, len(fr), ifidx, window, what="slot %d" % slot)
    assert npass(got) > 100


# ---- direction, keys ---------------------------------------------------------------------------

def test_direction(ctx):
    """br2's fuzz frames (internal and external ones mixed): the set, a NULL ifindex array, an empty
    set."""
    b = R.batch("br2", False)
    n = 500
    frames, lens, ifidx = reslot(b.frames[:n], 256), np.array(b.lens[:n]), np.array(b.ifidx[:n])
    iset = R.internal_ifindices(b.cfg)
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset)
    with_set, _, _ = check(ctx, frames, lens, n, ifidx, 128, what="set")
    null_ifx, _, _ = check(ctx, frames, lens, n, None, 128, what="null ifindex")
    ctx.set_internal_ifindices([])
    empty, _, _ = check(ctx, frames, lens, n, ifidx, 128, what="empty set")
    assert np.array_equal(null_ifx, empty) and (with_set != empty).any()
    want, _ = H.oracle(frames, lens, n, np.isin(ifidx, iset), *key1(), hfv.KEYSEL_ZERO)
    assert np.array_equal(with_set, want)


@pytest.mark.parametrize("window", [64, 128, 256])
def test_keysel_ifid(ctx, window):
    frames, lens, ifidx, _ = H.corpus()
    ctx.key_add_batch(0, ifid_raw())
    ctx.set_keysel(hfv.KEYSEL_IFID)
    ctx.set_internal_ifindices(iset1())
    want = cached("want1", lambda: corpus_want(hfv.KEYSEL_IFID))
    got, _, _ = check(ctx, frames, lens, len(frames), ifidx, window, want=want, what="ifid")
    assert npass(got) > 100


def test_keysel_ifid_one_slot_removed(ctx):
    frames, lens, ifidx, _ = H.corpus()
    ctx.key_add_batch(0, ifid_raw())
    ctx.set_keysel(hfv.KEYSEL_IFID)
    full, _, _ = check(ctx, frames, lens, len(frames), None, 128, what="ifid, full table")
    ctx.key_remove(1)
    hk, valid = orc.key_table(ifid_raw())
    part = valid.copy()
    part[0] &= np.uint32(~0x2 & 0xFFFFFFFF)
    want = corpus_want(hfv.KEYSEL_IFID, (hk, part), with_set=False)
    got, _, _ = check(ctx, frames, lens, len(frames), None, 128, want=want, what="ifid, slot 1 removed")
    assert npass(got) < npass(full)


def test_keysel_zero_empty_slot_fails_closed(ctx):
    """Slot 0 added, then removed: every bit clear, the status still right, as many frames run again."""
    frames, lens, ifidx, _ = H.corpus()
    n = len(frames)
    ctx.key_add(0, K1)
    _, st_key, r_key = check(ctx, frames, lens, n, ifidx, 128, what="with key")
    ctx.key_remove(0)
    got, st, retried = check(ctx, frames, lens, n, ifidx, 128, what="no key")
    assert not got.any() and np.array_equal(st, st_key) and retried == r_key > 0


def test_status_is_optional(ctx):
    frames, lens, ifidx, _ = H.corpus()
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    got, st, retried = check(ctx, frames, lens, len(frames), ifidx, 128, what="no status", status=False,
                             want=(cached("want0", corpus_want)[0], None))
    assert st is None and retried > 0


def test_key_change_between_two_calls(ctx):
    frames, lens, ifidx = tail(400)
    ctx.key_add(0, K1)
    first, _, _ = check(ctx, frames, lens, 400, ifidx, 128, what="key 1")
    ctx.key_add(0, bytes(range(16)))
    second, _, _ = check(ctx, frames, lens, 400, ifidx, 128, what="another key")
    assert npass(first) > 50 and not second.any()
    ctx.key_add(0, K1)
    third, _, _ = check(ctx, frames, lens, 400, ifidx, 128, what="key 1 again")
    assert np.array_equal(third, first)


def test_stops_a_running_service(ctx):
    frames, lens, ifidx = tail(400)
    ctx.key_add(0, K1)
    jw, js = judge(ctx, frames, lens, 400, ifidx)
    ctx.service_start()
    assert ctx.service_running
    got, st, _ = run_host(ctx, frames, lens, 400, ifidx, 128)
    assert not ctx.service_running
    assert np.array_equal(got, jw) and np.array_equal(st, js) and npass(got) > 50


# ---- arguments ---------------------------------------------------------------------------------

def test_arguments(ctx):
    frames, lens, ifidx = tail(64)
    fr = frames.reshape(-1).copy()
    bits = np.full(2, BITS_FILL, np.uint64)
    st = np.full(64, ST_FILL, np.uint8)
    L, h, E = hfv.lib(), ctx._h, -errno.EINVAL
    r = ctypes.c_size_t(77)

    def call(f, slot, ln, n, window, b):
        return L.hfv_verify_frames_host(h, f, slot, ln, ifidx.ctypes.data, n, window, st.ctypes.data, b, ctypes.byref(r))

    f, l, w = fr.ctypes.data, lens.ctypes.data, bits.ctypes.data
    assert call(None, SLOT, l, 64, 0, w) == E
    assert call(f, SLOT, None, 64, 0, w) == E
    assert call(f, SLOT, l, 64, 0, None) == E
    assert call(f, SLOT, l, 64, 0, w + 4) == E                # bitmap not 8-byte aligned
    assert call(f, 56, l, 64, 0, w) == E                      # slot < 64
    assert call(f, SLOT + 4, l, 64, 0, w) == E                # slot % 8
    assert call(f, 65536 * 8, l, 64, 0, w) == E               # slot > 65535 * 8
    assert call(f, SLOT, l, 64, 56, w) == E                   # window < 64
    assert call(f, SLOT, l, 64, 132, w) == E                  # window % 8
    assert call(f, SLOT, l, 64, SLOT + 8, w) == E             # window > slot
    assert call(None, SLOT, None, 0, 0, None) == 0            # n == 0: nothing to do, nothing touched
    assert call(f, SLOT, l, 0, 0, w) == 0
    assert r.value == 77 and (bits == np.uint64(BITS_FILL)).all() and (st == ST_FILL).all()


# ---- grids -------------------------------------------------------------------------------------

def test_capped_grids(request, ctx):
    """1, 2 and 3 blocks: the waves of a block claim the windowed kernel's tiles one after another."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    frames, lens, ifidx, _ = H.corpus()
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    want = cached("want0", corpus_want)
    try:
        for blocks in (1, 2, 3):
            hfv.Ctx.debug_batch_grid(blocks)
            for window in (120, 128):
                check(ctx, frames, lens, len(frames), ifidx, window, want=want, what="cap %d" % blocks)
    finally:
        hfv.Ctx.debug_batch_grid(0)


def test_real_grid(ctx):
    """More tiles than one block's waves: the corpus four times over, so that several blocks run."""
    frames, lens, ifidx, _ = H.corpus()
    fr, ln, ix = np.concatenate([frames] * 4), np.concatenate([lens] * 4), np.concatenate([ifidx] * 4)
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset1())
    w0, s0 = cached("want0", corpus_want)
    n = len(frames)
    got, st, _ = check(ctx, fr, ln, len(fr) - 27, ix, 128, what="real grid")
    assert np.array_equal(st[:n], s0) and np.array_equal(st[n:2 * n], s0)
    assert np.array_equal(hfv.bits_to_bool(got, len(fr) - 27)[:n], hfv.bits_to_bool(w0, n))
