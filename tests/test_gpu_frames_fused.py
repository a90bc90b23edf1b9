"""hfv_verify_frames_fused on the GPU: frames in, verdict bits out, in one launch.

Judges, all independent of the code under test: hfv_frame_extract per frame on the host (the parse of
hfv_frame_locate, and for frames from the internal link the host normalisation) with the record
checker orc.verify_records over the gathered fields, ANDed with status == 0 (oracle()); and the
router oracle on the frames whose verdict the hop-field check decides.  Bit-equality with the
three-launch hfv_verify_frames_rx is asserted beside one of those, never alone.

Every bitmap is pre-filled with a non-zero pattern and one guard word longer than needed; a status
buffer is pre-filled and three guard bytes longer; the frames (and the ifindex array) are compared
unchanged afterwards.  Integer work: every comparison is bit-exact.

The dealing tests cap the launch at 1, 2 or 3 blocks with the test build's hfv_debug_batch_grid and
run in a child process on lib/libscionhfv_test.so (conftest.rerun_on_test_build).

`make fusededge` builds three libraries with one wrong step each (csrc/hfv_frames_fused_kernel.hip);
this module must fail on every one, by assertions alone: run it with
HFV_LIB=lib/libscionhfv_fusededgeN.so HFV_TEST_BUILD_CHILD=1."""
import ctypes
import errno

import numpy as np
import pytest

import br_fuzz as F
import br_shift as S
import br_topo as T
import frames_rx_ref as R
import fused_deal as FD
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build
from test_gpu_frames import reslot
from test_gpu_frames_rx import dev, dev_ifx, dev_lens, run_verify_frames_rx

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = hfv.VERDICT
MAC = R.MAC
BITS_FILL = 0xC3A5C3A5C3A5C3A5     # neither 0 nor all-ones: a word never stored cannot pass for a verdict word
ST_FILL = 0x5A                     # no status value
ST_GUARD = 3
K1 = T.KEYS[1]


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)                  # a fresh ctx: default keysel, no keys, empty set
    yield c
    c.synchronize()
    c.close()


@pytest.fixture()
def cap():
    """Sets the block cap of the launch; the default geometry is back afterwards."""
    yield hfv.Ctx.debug_batch_grid
    if hasattr(hfv.lib(), "hfv_debug_batch_grid"):   # (the parent process runs on the product library)
        hfv.Ctx.debug_batch_grid(0)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def key1():
    return cached("key1", lambda: orc.key_table(K1))


def ifid_raw():
    """The table of test_verify_frames_keysel_ifid_256_keys: 256 generated keys, the topology's AS
    interfaces 1..6 under the AS key."""
    def make():
        raw = bytearray(orc.gen_key_table(256))
        for ifid in range(1, 7):
            raw[16 * ifid:16 * ifid + 16] = K1
        return bytes(raw)
    return cached("ifid_raw", make)


def oracle(frames, lens, n, internal, hop_keys, valid, keysel):
    """(bitmap words, status) of the first n frames by hfv_frame_extract per frame and the record
    checker; `internal` is a bool per frame (or one for all)."""
    internal = np.asarray(internal, dtype=bool)
    internal = internal[:n] if internal.ndim else np.broadcast_to(internal, (n,))
    st, inf, hf = R.frame_extract(np.ascontiguousarray(frames[:n]), lens[:n], internal)
    return R.oracle_bits(st, inf, hf, hop_keys, valid, keysel), st


def fill_words(count):
    return torch.from_numpy(np.full(count, BITS_FILL, dtype=np.uint64).view(np.int64)).to(DEV)


def run_fused(ctx, frames, lens, n, ifidx=None, status=True, d_frames=None, stream=None, timed=False):
    """The fused call over the first n frames.  Returns (words[(n+63)/64], status[n] or None, ms) and
    checks the guard word, the status guard bytes, and that frames and ifindex went unwritten."""
    slot = frames.shape[1]
    d = dev(frames) if d_frames is None else d_frames
    dl = dev_lens(lens)
    di = None if ifidx is None else dev_ifx(ifidx)
    words = (n + 63) // 64
    bits = fill_words(words + 1)
    st = torch.full((n + ST_GUARD,), ST_FILL, dtype=torch.uint8, device=DEV) if status else None
    call = ctx.verify_frames_fused_timed if timed else ctx.verify_frames_fused
    ms = call(d, slot, dl, n, bits, ingress_ifindex=di, status=st, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(frames.shape), frames), "frames were written"
    if di is not None:
        assert np.array_equal(di.cpu().numpy().view(np.uint32), np.asarray(ifidx, dtype=np.uint32)), "ifindex written"
    w = bits.cpu().numpy().view(np.uint64)
    assert w[words] == np.uint64(BITS_FILL), "wrote past the bitmap"
    got_st = None
    if status:
        got_st = st.cpu().numpy()
        assert (got_st[n:] == ST_FILL).all(), "wrote status past n"
        got_st = got_st[:n]
    return w[:words], got_st, ms


def check(ctx, frames, lens, n, ifidx, iset, keys, keysel, three=True, d_frames=None, what=""):
    """The fused call against the oracle (and beside it against the three-launch call).  The ctx
    already holds the keys and keysel; the set is installed here.  Returns (want words, status)."""
    ctx.set_internal_ifindices(iset)
    internal = np.isin(ifidx, iset) if ifidx is not None and len(iset) else False
    want, want_st = oracle(frames, lens, n, internal, keys[0], keys[1], keysel)
    got, got_st, _ = run_fused(ctx, frames, lens, n, ifidx, d_frames=d_frames)
    assert np.array_equal(got_st, want_st), ("status", what)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, "%d bad words, first %d: got %016x want %016x" % (
        len(bad), bad[0] if len(bad) else -1, int(got[bad[0]]) if len(bad) else 0, int(want[bad[0]]) if len(bad) else 0))
    if n % 64:
        assert int(got[-1]) >> (n % 64) == 0, "a bit at or past n is set"
    if three and d_frames is None:
        if ifidx is None:
            tw, ts = run_verify_frames_rx(ctx, frames[:n], lens[:n], None, n, rx=False)
        else:
            tw, ts = run_verify_frames_rx(ctx, frames[:n], lens[:n], ifidx[:n], n)
        assert np.array_equal(got, tw) and np.array_equal(got_st, ts), ("three-launch call", what)
    return want, want_st


def npass(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


# ---- fuzz parity, router oracle ----------------------------------------------------------------

FUZZ = [(b, v) for b in ("br1", "br2") for v in (False, True)]
FUZZ_IDS = ["%s-%s" % (b, "ipv6" if v else "ipv4") for b, v in FUZZ]


@pytest.mark.parametrize("br,v6", FUZZ, ids=FUZZ_IDS)
def test_fuzz_parity_keysel_zero(ctx, br, v6):
    """The 4096-frame fuzz batches, every frame external (no ifindex array)."""
    b = R.batch(br, v6)
    ctx.key_add(0, K1)
    want, st = check(ctx, b.frames, b.lens, 4096, None, [], key1(), hfv.KEYSEL_ZERO, what=(br, v6))
    assert 500 < npass(want) < (st == 0).sum()               # both verdicts among the parsed frames
    for s in (0, 17, 26, 34):
        assert (st == s).any(), s


@pytest.mark.parametrize("br,v6", FUZZ, ids=FUZZ_IDS)
def test_vs_router_oracle(ctx, br, v6):
    """Frames that reach the router on an external interface and whose verdict the hop-field check
    decides: the pass bit is the router oracle's SCION_FORWARD."""
    b = R.batch(br, v6)
    sel = b.sel_ext
    assert sel.sum() >= 1000 and (b.verdict[sel] == V["INVALID_HF"]).sum() >= 40
    ctx.key_add(0, K1)
    got, st, _ = run_fused(ctx, b.frames, b.lens, 4096)
    bits = hfv.bits_to_bool(got, 4096)
    assert (st[sel] == 0).all()
    assert np.array_equal(bits[sel], b.forward[sel])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4001])
def test_counts(ctx, n):
    """The last tile's clamp and the bits at and past n.  The last frame is one that passes, so a
    lane past n that voted with the clamped frame would set a bit at or past n."""
    b = R.batch("br2", False)
    ctx.key_add(0, K1)
    full, _ = oracle(b.frames, b.lens, 4096, False, *key1(), hfv.KEYSEL_ZERO)
    good = int(np.nonzero(hfv.bits_to_bool(full, 4096))[0][0])
    frames, lens = np.array(b.frames[:n + 3]), np.array(b.lens[:n + 3])
    frames[n - 1], lens[n - 1] = b.frames[good], b.lens[good]
    want, _ = check(ctx, frames, lens, n, None, [], key1(), hfv.KEYSEL_ZERO, what=n)
    assert (int(want[-1]) >> ((n - 1) % 64)) & 1 == 1


# ---- direction ---------------------------------------------------------------------------------

@pytest.mark.parametrize("br,v6", R.CASES[2:], ids=R.IDS[2:])
def test_direction_vs_record_and_router_oracle(ctx, br, v6):
    """The mixes of test_gpu_frames_rx.py: internal ifindices in the set, Cons 0 and 1.  With the set
    given the good internal Cons = 0 frames pass; without it they fail."""
    b = R.batch(br, v6)
    R.check_selection_counts(b, br)
    iset = R.internal_ifindices(b.cfg)
    ctx.key_add(0, K1)
    want, st = check(ctx, b.frames, b.lens, 4096, b.ifidx, iset, key1(), hfv.KEYSEL_ZERO, what=(br, v6))
    bits = hfv.bits_to_bool(want, 4096)                      # (= the fused call's words: check() asserted it)
    assert (st[b.sel] == 0).all()
    assert np.array_equal(bits[b.sel], b.forward[b.sel])
    good = b.sel_int & ~b.cons & b.forward
    assert good.sum() >= 500 and bits[good].all()
    # an empty set, and no ifindex array: every frame external
    plain, _ = oracle(b.frames, b.lens, 4096, False, *key1(), hfv.KEYSEL_ZERO)
    for name, s, ifx in (("empty set", [], b.ifidx), ("null ifindex", iset, None)):
        ctx.set_internal_ifindices(s)
        got, got_st, _ = run_fused(ctx, b.frames, b.lens, 4096, ifx)
        assert np.array_equal(got, plain) and np.array_equal(got_st, st), name
    pbits = hfv.bits_to_bool(plain, 4096)
    assert (pbits[good] == 0).sum() >= 500                   # the ingress rule misjudges them


def test_direction_set_changed_between_enqueued_calls(ctx):
    """The set is host state copied into each launch's arguments: a call enqueued before a change
    keeps the set it was enqueued with.  Two calls on one stream behind a sleep, one synchronize."""
    b = R.batch("br2", False)
    iset = R.internal_ifindices(b.cfg)
    ctx.key_add(0, K1)
    with_set, _ = oracle(b.frames, b.lens, 4096, b.internal, *key1(), hfv.KEYSEL_ZERO)
    plain, _ = oracle(b.frames, b.lens, 4096, False, *key1(), hfv.KEYSEL_ZERO)
    assert (with_set != plain).sum() >= 10
    d, dl, di = dev(b.frames), dev_lens(b.lens), dev_ifx(b.ifidx)
    outs = [fill_words(65) for _ in range(3)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(5_000_000)
    ctx.set_internal_ifindices(iset)
    ctx.verify_frames_fused(d, b.frames.shape[1], dl, 4096, outs[0], ingress_ifindex=di, stream=s)
    ctx.set_internal_ifindices([])
    ctx.verify_frames_fused(d, b.frames.shape[1], dl, 4096, outs[1], ingress_ifindex=di, stream=s)
    ctx.set_internal_ifindices(iset)
    ctx.verify_frames_fused(d, b.frames.shape[1], dl, 4096, outs[2], ingress_ifindex=di, stream=s)
    s.synchronize()
    for o, w in zip(outs, (with_set, plain, with_set)):
        got = o.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:64], w) and got[64] == np.uint64(BITS_FILL)


# ---- window edges ------------------------------------------------------------------------------

FAMILIES = pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])


@FAMILIES
@pytest.mark.parametrize("slot", [256, 136], ids=["staged", "direct"])
def test_window_edge_corpus_and_sweep(ctx, slot, v6):
    """br_shift's corpus and truncation sweep: PathMeta, SegIDs, hop field and MAC in front of,
    across and past bytes 128 and 136, with each BR's internal interfaces as the set.  In 136-byte
    slots the longer frames are cut by the slot."""
    ctx.key_add(0, K1)
    parsed = passed = 0
    for name, br, fam, frames, lens, ifidx in S.fixture_legs():
        if fam != v6:
            continue
        iset = R.internal_ifindices(T.br_config(br, v6))
        want, st = check(ctx, reslot(frames, slot), lens, len(frames), ifidx, iset, key1(), hfv.KEYSEL_ZERO, what=name)
        if name.startswith("corpus") and slot == 256:
            assert (st == 0).all()
        parsed += int((st == 0).sum())
        passed += npass(want)
    assert parsed >= (400 if slot == 256 else 100) and passed >= (200 if slot == 256 else 20)


@FAMILIES
def test_window_edge_corpus_vs_router_oracle(ctx, v6):
    """The br1 corpus and a copy with one MAC bit flipped per frame: for the frames from an external
    interface the pass bit is the router oracle's SCION_FORWARD."""
    frames, lens, ifidx, _, _ = S.shift_corpus(v6)["br1"]
    bad = frames.copy()
    for i in range(len(bad)):
        bad[i, S.field_offsets(bytes(frames[i]))["mac"][0] + i % 6] ^= 1 << (i % 8)
    frames, lens, ifidx = np.concatenate([frames, bad]), np.concatenate([lens, lens]), np.concatenate([ifidx, ifidx])
    cfg = T.br_config("br1", v6)
    _, verdict, _, _ = orc.br_process(frames.copy(), lens, ifidx, cfg, orc.hop_key(K1))
    sel = ~np.isin(ifidx, R.internal_ifindices(cfg)) & np.isin(verdict, [V["SCION_FORWARD"], V["INVALID_HF"]])
    n = len(frames)
    assert sel.sum() >= n // 3 and (verdict[sel] == V["INVALID_HF"]).sum() == sel.sum() // 2
    ctx.key_add(0, K1)
    got, st, _ = run_fused(ctx, frames, lens, n)
    assert (st == 0).all()
    assert np.array_equal(hfv.bits_to_bool(got, n)[sel], verdict[sel] == V["SCION_FORWARD"])


def test_long_paths_and_options_shift(ctx):
    """The hop field past the staged window, the cut one byte short of its end (status 17), and the
    IPv4 options that move every header."""
    ctx.key_add(0, K1)
    frames, lens, _, m = F.options_shift_batch(R.hop_inputs(False))
    want, st = check(ctx, frames, lens, len(frames), None, [], key1(), hfv.KEYSEL_ZERO, what="options shift")
    assert (st == 0).all() and len(frames) == 11 * m and npass(want) >= m
    for v6 in (False, True):
        frames, lens = T.to_slots([f for f, _ in F.long_path_frames(v6, MAC)])
        want, st = check(ctx, frames, lens, len(frames), None, [], key1(), hfv.KEYSEL_ZERO, what="long paths")
        assert (st == 0).all()
        cut = np.array([hfv.frame_locate(bytes(frames[i, :lens[i]]))[2] + 11 for i in range(len(frames))], np.uint16)
        assert (cut > 256).all()
        want, st = check(ctx, frames, cut, len(frames), None, [], key1(), hfv.KEYSEL_ZERO, what="long paths, cut")
        assert (st == 17).all() and not want.any()


# ---- slots and alignment -----------------------------------------------------------------------

@pytest.mark.parametrize("slot", [144, 256, 2048, 136, 64])
def test_slots(ctx, slot):
    """144 is the loop's ring slot; 136 and 64 take the kernel without 16-byte staging loads."""
    b = R.batch("br3", slot >= 144)                          # IPv6 where its headers fit the slot
    ctx.key_add(0, K1)
    want, st = check(ctx, reslot(b.frames, slot), b.lens, 4096, b.ifidx, R.internal_ifindices(b.cfg), key1(),
                     hfv.KEYSEL_ZERO, what=slot)
    if slot >= 136:
        assert (st == 0).sum() >= 1000 and npass(want) >= 500
    else:
        assert not want.any()                                # slot 64 ends inside the SCION header


def test_misaligned_frame_buffer(ctx):
    """A frame buffer that is 8- but not 16-byte aligned (the unstaged kernel)."""
    b = R.batch("br2", False)
    slot, n = 256, 1000
    fr = reslot(b.frames[:n], slot)
    buf = torch.zeros(n * slot + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[8:8 + n * slot]
    view.copy_(torch.from_numpy(fr.reshape(-1)))
    ctx.key_add(0, K1)
    want, st = check(ctx, fr, b.lens, n, b.ifidx, R.internal_ifindices(b.cfg), key1(), hfv.KEYSEL_ZERO, d_frames=view)
    assert npass(want) >= 100


# ---- keys --------------------------------------------------------------------------------------

def test_keysel_ifid_256_keys(ctx):
    b = R.batch("br3", True)
    ctx.key_add_batch(0, ifid_raw())
    ctx.set_keysel(hfv.KEYSEL_IFID)
    keys = cached("ifid_keys", lambda: orc.key_table(ifid_raw()))
    want, _ = check(ctx, b.frames, b.lens, 4096, b.ifidx, R.internal_ifindices(b.cfg), keys, hfv.KEYSEL_IFID)
    assert npass(want) > 500
    b = R.batch("br1", False)                                # every frame external, another family
    want, _ = check(ctx, b.frames, b.lens, 4001, None, [], keys, hfv.KEYSEL_IFID)
    assert npass(want) > 500


def test_keysel_ifid_partial_table(ctx):
    """The frames' slots (the AS interfaces 1..6) missing from the table: those bits are 0."""
    b = R.batch("br1", True)
    ctx.key_add_batch(0, ifid_raw())
    for k in range(1, 7):
        ctx.key_remove(k)
    ctx.set_keysel(hfv.KEYSEL_IFID)
    hk, valid = cached("ifid_keys", lambda: orc.key_table(ifid_raw()))
    full, _ = oracle(b.frames, b.lens, 4096, False, hk, valid, hfv.KEYSEL_IFID)
    assert npass(full) > 500
    part = valid.copy()
    part[0] &= np.uint32(~0x7E & 0xFFFFFFFF)
    want, st = check(ctx, b.frames, b.lens, 4096, None, [], (hk, part), hfv.KEYSEL_IFID)
    assert not want.any() and (st == 0).sum() > 2000


def test_keysel_zero_without_key_fails_closed(ctx):
    """Slot 0 added, then removed: no bit set, the status still exact."""
    b = R.batch("br2", False)
    ctx.key_add(0, K1)
    ctx.key_remove(0)
    hk, valid = key1()
    want, st = check(ctx, b.frames, b.lens, 4001, b.ifidx, R.internal_ifindices(b.cfg), (hk, np.zeros(8, np.uint32)),
                     hfv.KEYSEL_ZERO)
    assert not want.any() and (st == 0).sum() > 3000


# ---- optional status, timed form, arguments ----------------------------------------------------

def test_status_is_optional(ctx):
    b = R.batch("br2", True)
    iset = R.internal_ifindices(b.cfg)
    ctx.key_add(0, K1)
    want, _ = check(ctx, b.frames, b.lens, 4001, b.ifidx, iset, key1(), hfv.KEYSEL_ZERO)
    got, st, _ = run_fused(ctx, b.frames, b.lens, 4001, b.ifidx, status=False)
    assert st is None and np.array_equal(got, want) and npass(want) > 500


def test_timed_form(ctx):
    b = R.batch("br1", False)
    ctx.key_add(0, K1)
    want, _ = oracle(b.frames, b.lens, 4096, False, *key1(), hfv.KEYSEL_ZERO)
    got, _, ms = run_fused(ctx, b.frames, b.lens, 4096, timed=True)
    assert 0.0 < ms < 100.0
    assert np.array_equal(got, want) and npass(want) > 500
    # n == 0: 0.0, and nothing touched
    bits, st = fill_words(2), torch.full((8,), ST_FILL, dtype=torch.uint8, device=DEV)
    assert ctx.verify_frames_fused_timed(dev(b.frames[:8]), b.frames.shape[1], dev_lens(b.lens[:8]), 0, bits,
                                         status=st) == 0.0
    torch.cuda.synchronize()
    assert (bits.cpu().numpy().view(np.uint64) == np.uint64(BITS_FILL)).all() and (st == ST_FILL).all()


def test_arguments(ctx):
    b = R.batch("br2", False)
    n, slot = 64, b.frames.shape[1]
    d, dl, di = dev(b.frames[:n]), dev_lens(b.lens[:n]), dev_ifx(b.ifidx[:n])
    status = torch.full((n,), 0x77, dtype=torch.uint8, device=DEV)
    bits = torch.full((2,), 0x77, dtype=torch.int64, device=DEV)
    L, h = hfv.lib(), ctx._h
    ms = ctypes.c_float(-1.0)

    def both(frames_p, slot_, len_p, n_, status_p, bits_p):
        a = L.hfv_verify_frames_fused(h, frames_p, slot_, len_p, di.data_ptr(), n_, status_p, bits_p, None)
        c = L.hfv_verify_frames_fused_timed(h, frames_p, slot_, len_p, di.data_ptr(), n_, status_p, bits_p, None,
                                            ctypes.byref(ms))
        assert a == c
        return a

    f, l, s, w = d.data_ptr(), dl.data_ptr(), status.data_ptr(), bits.data_ptr()
    E = -errno.EINVAL
    assert both(f, slot + 4, l, n, s, w) == E                # slot % 8
    assert both(f, 56, l, n, s, w) == E                      # slot < 64
    assert both(f, (1 << 24) + 8, l, n, s, w) == E           # slot > 16 MiB
    assert both(f, slot, l, (1 << 36) + 1, s, w) == E        # n > 2^36
    assert both(None, slot, l, n, s, w) == E
    assert both(f, slot, None, n, s, w) == E
    assert both(f, slot, l, n, s, None) == E
    assert both(f, slot, l, n, s, w + 4) == E                # bitmap not 8-byte aligned
    assert L.hfv_verify_frames_fused(None, f, slot, l, di.data_ptr(), n, s, w, None) == E
    assert L.hfv_verify_frames_fused_timed(h, f, slot, l, di.data_ptr(), n, s, w, None, None) == E
    # n == 0: nothing to do, nothing written, even with null buffers
    assert both(None, slot, None, 0, None, None) == 0 and ms.value == 0.0
    assert both(f, slot, l, 0, s, w) == 0
    torch.cuda.synchronize()
    assert (status == 0x77).all() and (bits == 0x77).all()


# ---- stream order, key publication -------------------------------------------------------------

def test_stream_ordered(ctx):
    """H2D copies of the frames, lengths and ifindices (behind a few ms of other work), the fused call
    and a torch consumer of the bitmap on one non-default stream, one synchronize at the end."""
    parts = [R.batch(br, False) for br in ("br2", "br3", "br2", "br3", "br2")]
    frames = np.concatenate([p.frames for p in parts])[:20000]
    lens = np.concatenate([p.lens for p in parts])[:20000]
    ifidx = np.concatenate([p.ifidx for p in parts])[:20000]
    n, slot = frames.shape
    iset = sorted(set(R.internal_ifindices(parts[0].cfg)) | set(R.internal_ifindices(parts[1].cfg)))
    ctx.key_add(0, K1)
    ctx.set_internal_ifindices(iset)
    want, _ = oracle(frames, lens, n, np.isin(ifidx, iset), *key1(), hfv.KEYSEL_ZERO)
    plain, _ = oracle(frames, lens, n, False, *key1(), hfv.KEYSEL_ZERO)
    assert (want != plain).sum() >= 100                      # the ifindex copy matters to the result
    host = torch.from_numpy(np.array(frames, copy=True)).pin_memory()
    hlens = torch.from_numpy(np.array(lens, copy=True).view(np.int16)).pin_memory()
    hifx = torch.from_numpy(np.array(ifidx, copy=True).view(np.int32)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.zeros((n, slot), dtype=torch.uint8, device=DEV)
        dl = torch.zeros(n, dtype=torch.int16, device=DEV)
        di = torch.zeros(n, dtype=torch.int32, device=DEV)
        bits = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=DEV)
        torch.cuda._sleep(5_000_000)                         # the producer runs late
        d.copy_(host, non_blocking=True)
        dl.copy_(hlens, non_blocking=True)
        di.copy_(hifx, non_blocking=True)
        ctx.verify_frames_fused(d, slot, dl, n, bits, ingress_ifindex=di, stream=s)
        out = bits.clone()                                   # the consumer
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("keysel", [hfv.KEYSEL_ZERO, hfv.KEYSEL_IFID], ids=["zero", "ifid"])
def test_key_publication(ctx, keysel):
    """Two fused calls on one stream held behind a sleep, a key_add of another key between them: each
    call's bitmap is the one of the key it was enqueued with.  Under KEYSEL_ZERO the key travels in
    the launch's arguments; under KEYSEL_IFID the first launch reads the device table it was launched
    with while the host already publishes the next one (the event behind the first call is asserted
    pending once the second is enqueued).  A third bitmap holds the warm-up call's verdicts."""
    from test_gpu_key_publish import Window
    b = R.batch("br1", False)
    n, slot = 4096, b.frames.shape[1]
    other = bytes(range(16))
    tables = []
    for key in (K1, other):
        raw = bytearray(ifid_raw())
        for ifid in range(0 if keysel == hfv.KEYSEL_ZERO else 1, 7):
            raw[16 * ifid:16 * ifid + 16] = key
        tables.append(bytes(raw))
    wants = [oracle(b.frames, b.lens, n, False, *orc.key_table(t), keysel)[0] for t in tables]
    assert npass(wants[0]) > 500 and not wants[1].any()
    ctx.set_keysel(keysel)
    ctx.key_add_batch(0, tables[0])
    d, dl = dev(b.frames), dev_lens(b.lens)
    outs = [fill_words(65) for _ in range(3)]
    s = torch.cuda.Stream()
    ctx.verify_frames_fused(d, slot, dl, n, outs[2], stream=s)   # warm-up: table 0 is published
    w = Window(s)
    w.open()
    ctx.verify_frames_fused(d, slot, dl, n, outs[0], stream=s)
    w.mark()
    for ifid in range(0 if keysel == hfv.KEYSEL_ZERO else 1, 7):
        ctx.key_add(ifid, other)
    ctx.verify_frames_fused(d, slot, dl, n, outs[1], stream=s)
    w.assert_open()
    w.report("fused key publication")
    for o, want in zip(outs, (wants[0], wants[1], wants[0])):
        got = o.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:64], want) and got[64] == np.uint64(BITS_FILL)


# ---- tile dealing ------------------------------------------------------------------------------

CYCLE = 4001     # frames of the cycled batch: odd, so no two tiles of a call start at the same frame


def deal_case(keysel):
    """(frames [CYCLE, 256], lens, passes bool[CYCLE]) judged once on the host."""
    def make():
        b = R.batch("br1", False)
        frames, lens = reslot(b.frames[:CYCLE], 256), np.array(b.lens[:CYCLE])
        keys = key1() if keysel == hfv.KEYSEL_ZERO else orc.key_table(ifid_raw())
        words, _ = oracle(frames, lens, CYCLE, False, keys[0], keys[1], keysel)
        return frames, lens, hfv.bits_to_bool(words, CYCLE)
    return cached(("deal", keysel), make)


def deal_expected(passes, n):
    """The words of n frames cycled from the batch.  Checked here, on the CPU: every full tile's word
    is neither 0 nor all-ones nor the bitmap's fill, and differs from its neighbours' -- so a word
    that was dropped, or stored from another tile, cannot pass for the right one."""
    p = passes[np.arange(n) % CYCLE].astype(np.uint8)
    words = np.packbits(np.concatenate([p, np.zeros(-n % 64, np.uint8)]), bitorder="little").view(np.uint64)
    full = words[:n // 64]
    assert not (full == 0).any() and not (full == np.uint64(2**64 - 1)).any() and not (full == np.uint64(BITS_FILL)).any()
    assert (full[1:] != full[:-1]).all()
    assert words[-1] != 0 or n % 64 == 0
    return words


def run_deal(ctx, keysel, blocks, what):
    frames, lens, passes = deal_case(keysel)
    n = FD.deal_n(keysel, blocks)
    want = deal_expected(passes, n)
    i = torch.arange(n, device=DEV) % CYCLE
    d = torch.from_numpy(frames).to(DEV)[i].contiguous()
    dl = dev_lens(lens)[i].contiguous()
    words = (n + 63) // 64
    bits = fill_words(words + 1)
    st = torch.full((n + ST_GUARD,), ST_FILL, dtype=torch.uint8, device=DEV)
    ctx.verify_frames_fused(d, 256, dl, n, bits, status=st)
    torch.cuda.synchronize()
    got = bits.cpu().numpy().view(np.uint64)
    assert got[words] == np.uint64(BITS_FILL), ("wrote past the bitmap", what)
    bad = np.nonzero(got[:words] != want)[0]
    assert not len(bad), (what, "%d bad words of %d, first %d: got %016x want %016x" % (
        len(bad), words, bad[0], int(got[bad[0]]), int(want[bad[0]])))
    assert int(got[words - 1]) >> 37 == 0
    assert (st[n:] == ST_FILL).all() and not (st[:n] == ST_FILL).any()


def setup_deal(ctx, keysel):
    if keysel == hfv.KEYSEL_ZERO:
        ctx.key_add(0, K1)
    else:
        ctx.key_add_batch(0, ifid_raw())
    ctx.set_keysel(keysel)


@pytest.mark.parametrize("keysel", [hfv.KEYSEL_ZERO, hfv.KEYSEL_IFID], ids=["zero", "ifid"])
def test_tile_dealing_capped(request, ctx, cap, keysel):
    """1, 2 and 3 blocks: every wave claims five tiles or more, the block ranges are ragged and the
    last tile is partial (tests/fused_deal.py; test_frames_fused.py pins the shapes)."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    setup_deal(ctx, keysel)
    for blocks in FD.CAPS:
        cap(blocks)
        run_deal(ctx, keysel, blocks, (keysel, "cap %d" % blocks))


@pytest.mark.parametrize("keysel", [hfv.KEYSEL_ZERO, hfv.KEYSEL_IFID], ids=["zero", "ifid"])
def test_tile_dealing_real_grid(ctx, keysel):
    """One block per CU, five tiles per wave and one over."""
    blocks = torch.cuda.get_device_properties(0).multi_processor_count
    setup_deal(ctx, keysel)
    run_deal(ctx, keysel, blocks, (keysel, "real grid of %d" % blocks))
