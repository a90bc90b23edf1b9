"""hfv_verify_frames_desc on the GPU: frames addressed by descriptors into one buffer, verified in
place in one launch.

Two judges throughout, neither of them the code under test: the host judge (hfv_frame_extract on the
bytes each valid descriptor names, where they lie in the buffer, and the record checker:
test_frames_desc.host_judge), and Ctx.verify_frames_fused on the slot copy of the same frames
(frames_desc.slot_copy: the equivalence the header states).  Both must agree with the call, bit for
bit and status for status; an invalid descriptor gives status 255 and bit 0.

Every run pre-fills the bitmap with 0xC3A5C3A5C3A5C3A5 plus one guard word and the status with 0x5A
plus three guard bytes, and compares the whole buffer (its 4 KiB guard regions included) and the
descriptor array unchanged afterwards.  Integer work: every comparison is bit-exact.

The dealing tests cap the launch at 1, 2 or 3 blocks with the test build's hfv_debug_batch_grid and
run in a child process on lib/libscionhfv_test.so (conftest.rerun_on_test_build).

`make descedge` builds six libraries with one wrong step each (csrc/hfv_frames_desc_kernel.hip):
lib/libscionhfv_descedge1.so .. lib/libscionhfv_descedge6.so.  This module must fail on every one, by
assertions alone: run it with HFV_LIB=lib/libscionhfv_descedgeN.so HFV_TEST_BUILD_CHILD=1.  Every bad
address the tests use points into the module's own guard regions."""
import ctypes
import errno
import hashlib

import numpy as np
import pytest

import frames_desc as D
import frames_rx_ref as R
import fused_deal as FD
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build
from test_frames_desc import host_judge
from test_gpu_frames_fused import BITS_FILL, ST_FILL, ST_GUARD, K1, deal_case, deal_expected, ifid_raw, key1, npass
from test_gpu_frames_rx import dev, dev_ifx, dev_lens

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOTH = pytest.mark.parametrize("keysel", [hfv.KEYSEL_ZERO, hfv.KEYSEL_IFID], ids=["zero", "ifid"])


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


def ifid_keys():
    return cached("ifid_keys", lambda: orc.key_table(ifid_raw()))


def install(ctx, keysel):
    """The AS key in slot 0 (KEYSEL_ZERO) or the 256-key table (KEYSEL_IFID); returns (hop keys,
    valid words) for the judges."""
    if keysel == hfv.KEYSEL_ZERO:
        ctx.key_add(0, K1)
        return key1()
    ctx.key_add_batch(0, ifid_raw())
    ctx.set_keysel(hfv.KEYSEL_IFID)
    return ifid_keys()


def fill_words(count):
    return torch.from_numpy(np.full(count, BITS_FILL, dtype=np.uint64).view(np.int64)).to(DEV)


def to_device(buf, misalign=0):
    """The buffer on the device at an address = misalign mod 16 (frames_desc.GUARD is a multiple of
    16, so the UMEM proper has the same residue).  Returns the view holding it."""
    raw = torch.zeros(len(buf) + 32, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    view = raw[misalign:misalign + len(buf)]
    view.copy_(torch.from_numpy(np.array(buf, copy=True)))
    return view


def dev_desc(desc):
    return torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).copy()).to(DEV)


def run_desc(ctx, buf, off, nbytes, desc, n=None, status=True, misalign=0, stream=None, timed=False, d_buf=None):
    """The call over the first n descriptors.  Returns (words[(n+63)/64], status[n] or None, ms) and
    checks the guard word, the status guard bytes, and that the whole buffer and the descriptors went
    unwritten."""
    n = len(desc) if n is None else n
    d = to_device(buf, misalign) if d_buf is None else d_buf
    dd = dev_desc(desc)
    words = (n + 63) // 64
    bits = fill_words(words + 1)
    st = torch.full((n + ST_GUARD,), ST_FILL, dtype=torch.uint8, device=DEV) if status else None
    call = ctx.verify_frames_desc_timed if timed else ctx.verify_frames_desc
    ms = call(d.data_ptr() + off, nbytes, dd, n, bits, status=st, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), buf), "the buffer was written"
    assert dd.cpu().numpy().tobytes() == np.ascontiguousarray(desc).tobytes(), "descriptors written"
    w = bits.cpu().numpy().view(np.uint64)
    assert w[words] == np.uint64(BITS_FILL), "wrote past the bitmap"
    got_st = None
    if status:
        got_st = st.cpu().numpy()
        assert (got_st[n:] == ST_FILL).all(), "wrote status past n"
        got_st = got_st[:n]
    return w[:words], got_st, ms


def fused_judge(ctx, buf, off, nbytes, desc):
    """(words, status) of Ctx.verify_frames_fused on the slot copy, under the ctx's keys, keysel and
    set; the indices of invalid descriptors are set to (bit 0, status 255) as the header says."""
    frames, lens, ifidx, valid = D.slot_copy(buf, off, nbytes, desc)
    n = len(desc)
    words = (n + 63) // 64
    bits = fill_words(words)
    st = torch.full((n,), ST_FILL, dtype=torch.uint8, device=DEV)
    ctx.verify_frames_fused(dev(frames), frames.shape[1], dev_lens(lens), n, bits, ingress_ifindex=dev_ifx(ifidx),
                            status=st)
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    ok = hfv.bits_to_bool(bits.cpu().numpy().view(np.uint64), n) & valid
    st[~valid] = D.BAD_DESC
    return pack(ok), st


def pack(passes):
    p = np.asarray(passes, dtype=np.uint8)
    return np.packbits(np.concatenate([p, np.zeros(-len(p) % 64, np.uint8)]), bitorder="little").view(np.uint64)


def judges(ctx, buf, off, nbytes, desc, iset, keys, keysel, tag):
    """Both judges (computed once per distinct input per process); they must agree with each other
    before anything is held against them.  The ctx holds the keys and keysel; the set is installed
    here."""
    ctx.set_internal_ifindices(iset)
    h = hashlib.sha1()
    for a in (buf, desc):
        h.update(np.ascontiguousarray(a).tobytes())
    key = ("judge", h.hexdigest(), off, nbytes, tuple(iset), keysel, tag)

    def make():
        hw, hs = host_judge(buf, off, nbytes, desc, iset, keys[0], keys[1], keysel)
        fw, fs = fused_judge(ctx, buf, off, nbytes, desc)
        assert np.array_equal(hs, fs) and np.array_equal(hw, fw), "the two judges disagree"
        return hw, hs
    return cached(key, make)


def check(ctx, buf, off, nbytes, desc, iset, keys, keysel, tag="keys", what="", want=None, **kw):
    """The call against both judges.  Returns (want words, want status)."""
    want, want_st = judges(ctx, buf, off, nbytes, desc, iset, keys, keysel, tag) if want is None else want
    ctx.set_internal_ifindices(iset)
    n = len(desc)
    got, got_st, _ = run_desc(ctx, buf, off, nbytes, desc, **kw)
    bad_st = np.nonzero(got_st != want_st)[0]
    assert not len(bad_st), (what, "status: %d differ, first at %d: got %d want %d" % (
        len(bad_st), bad_st[0], got_st[bad_st[0]], want_st[bad_st[0]]))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, "%d bad words, first %d: got %016x want %016x" % (
        len(bad), bad[0], int(got[bad[0]]), int(want[bad[0]])))
    if n % 64:
        assert int(got[-1]) >> (n % 64) == 0, "a bit at or past n is set"
    return want, want_st


# ---- 1. parity ----------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("src", D.FUZZ + D.SHIFT)
def test_parity(ctx, src, keysel):
    """The six fuzz batches, br_shift's window-edge corpus and its truncation sweeps, in order, in
    recycled order and packed (every addr & 15), with the BR's internal interfaces as the set."""
    keys = install(ctx, keysel)
    iset = D.internal_set(src)
    for kind in D.KINDS:
        buf, off, nbytes, desc = D.corpus(src, kind)
        want, st = check(ctx, buf, off, nbytes, desc, iset, keys, keysel, what=(src, kind))
        assert (st == 0).sum() >= len(desc) // 8 and npass(want) >= len(desc) // 16
    if src.startswith("fuzz"):
        for s in (0, 17, 26, 34):
            assert (st == s).any(), s


# ---- 2. alignment sweep -------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(16))
def test_alignment_sweep(ctx, k):
    """br_shift's corpus (PathMeta, SegIDs, hop field and MAC in front of, across and past bytes 128
    and 136) with every frame at addr = k mod 16, through the staged kernel and, with the buffer one
    byte off 16-byte alignment, through the unstaged one."""
    keys = install(ctx, hfv.KEYSEL_ZERO)
    parsed = passed = 0
    for src in D.SHIFT_CORPUS:
        buf, off, nbytes, desc = D.corpus(src, ("shift", k))
        assert ((desc["addr"] & 15) == k).all()
        iset = D.internal_set(src)
        for misalign in (0, 1):
            want, st = check(ctx, buf, off, nbytes, desc, iset, keys, hfv.KEYSEL_ZERO, what=(src, k, misalign),
                             misalign=misalign)
        assert (st == 0).all()
        parsed += len(desc)
        passed += npass(want)
    assert parsed == 2592 and passed >= 1200


# ---- 3. tile edges ------------------------------------------------------------------------------

def big_case():
    """20000 frames of five fuzz batches, packed; read-only."""
    def make():
        parts = [R.batch(br, False) for br in ("br2", "br3", "br2", "br3", "br2")]
        frames = np.concatenate([p.frames for p in parts])[:20000]
        lens = np.concatenate([p.lens for p in parts])[:20000]
        ifidx = np.concatenate([p.ifidx for p in parts])[:20000]
        iset = sorted(set(R.internal_ifindices(parts[0].cfg)) | set(R.internal_ifindices(parts[1].cfg)))
        return D.layout(frames, lens, "packed", ifindex=ifidx) + (iset,)
    return cached("big", make)


@BOTH
def test_tile_edges(ctx, keysel):
    """n = 1 .. 20000 over one packed buffer: the last tile's clamp, the bits at and past n, one block
    and many.  The last descriptor of every run is one of a frame that passes, so a lane past n that
    voted with the repeated descriptor would set a bit at or past n."""
    keys = install(ctx, keysel)
    buf, off, nbytes, desc, iset = big_case()
    want, want_st = judges(ctx, buf, off, nbytes, desc, iset, keys, keysel, "keys")
    passes = hfv.bits_to_bool(want, len(desc))
    good = int(np.nonzero(passes)[0][0])
    assert npass(want) > 5000
    d_buf = to_device(buf)
    w = FD.WAVES[keysel]
    for n in sorted(set(FD.TEST_SIZES) | {w * 64 - 1, w * 64 + 1}):
        dn = desc[:n].copy()
        dn[n - 1] = desc[good]                               # (descriptors may repeat a frame)
        p, s = passes[:n].copy(), want_st[:n].copy()
        p[n - 1], s[n - 1] = True, 0
        check(ctx, buf, off, nbytes, dn, iset, keys, keysel, what=n, want=(pack(p), s), d_buf=d_buf)


# ---- 4. UMEM edges ------------------------------------------------------------------------------

@BOTH
def test_umem_edges(ctx, keysel):
    """A frame at addr 0; a frame shorter than 128 bytes that ends exactly at umem_bytes, at several
    addr & 15; an odd umem_bytes; a UMEM of one 64-byte frame.  Guards and gaps of zeros, of 0xFF, and
    of copies of a passing frame with the cut frame's own remaining bytes behind it: a read outside
    the frame, or outside the UMEM, would meet a frame that passes.  All three give the same output."""
    keys = install(ctx, keysel)
    frames, lens, ifidx = D.edge_source()
    passing = bytes(frames[0, :lens[0]])
    outs = {}
    for fname, filler, spill in (("zeros", 0, False), ("ones", 0xFF, False), ("frames", passing, True)):
        for name, buf, off, nbytes, desc in D.edge_cases(frames, lens, ifidx, filler=filler, spill=spill):
            for misalign in (0, 1):
                want, st = check(ctx, buf, off, nbytes, desc, [], keys, keysel, what=(name, fname, misalign),
                                 misalign=misalign)
                assert outs.setdefault(name, (want.tobytes(), st.tobytes())) == (want.tobytes(), st.tobytes())
            if name == "one64" or name in ("tail_0_60", "tail_7_100", "tail_8_64", "tail_15_77"):
                assert st[-1] != 0 and (int(want[0]) >> (len(desc) - 1)) & 1 == 0   # cut inside its header
            assert (st[:-1] == 0).all() and npass(want) >= len(desc) - 1


# ---- 5. bytes past len are absent ---------------------------------------------------------------

@pytest.mark.parametrize("src", D.FUZZ)
def test_bytes_past_len_are_absent(ctx, src):
    """One passing frame per fuzz batch, whole in memory, named by descriptors whose len runs from
    60 to its full length in steps of 4: status and bit are those of the frame cut at len."""
    keys = install(ctx, hfv.KEYSEL_ZERO)
    _, br, v6 = src.split("_")
    b = R.batch(br, bool(int(v6)))
    iset = D.internal_set(src)
    i = int(np.nonzero(b.sel & b.forward)[0][0])
    full = int(min(b.lens[i], b.frames.shape[1]))
    buf, off, nbytes, d1 = D.layout(b.frames[i:i + 1], b.lens[i:i + 1], "inorder", filler=0xFF, ifindex=b.ifidx[i:i + 1])
    cuts = list(range(60, full, 4)) + [full]
    desc = np.zeros(len(cuts), dtype=D.DTYPE)
    desc["addr"], desc["len"], desc["ifindex"] = d1["addr"][0], cuts, d1["ifindex"][0]
    hdr = hfv.frame_locate(bytes(b.frames[i, :full]))[2] + 12
    for misalign in (0, 1):
        want, st = check(ctx, buf, off, nbytes, desc, iset, keys, hfv.KEYSEL_ZERO, what=(src, misalign), misalign=misalign)
    ok = hfv.bits_to_bool(want, len(cuts))
    for c, s, o in zip(cuts, st, ok):
        assert (s == 0 and o) == (c >= hdr), (c, hdr, s, o)
    assert (np.array(cuts) < hdr).sum() >= 10 and ok[-1]


# ---- 6. bad descriptors -------------------------------------------------------------------------

def bad_case():
    """64 short passing frames in 2048-byte chunks (a UMEM of 128 KiB), a passing frame planted in
    the back guard at umem_bytes + 1 and one in the front guard at -8 (where addr = 2^64 - 8 points
    once the device adds it to the pointer), and 229 descriptors cycling over the frames."""
    def make():
        b = R.batch("br1", False)
        idx = np.nonzero(b.sel_ext & b.forward & (b.lens <= 240))[0][:64]
        assert len(idx) == 64
        frames, lens, ifidx = np.array(b.frames[idx]), np.array(b.lens[idx]), np.array(b.ifidx[idx])
        buf, off, nbytes, d = D.layout(frames, lens, "inorder", filler=0xFF, ifindex=ifidx)
        assert nbytes > 65536 + 2048
        planted = bytes(frames[0, :lens[0]])
        D.plant(buf, off, nbytes + 1, planted)
        D.plant(buf, off, (1 << 64) - 8, planted)            # ends inside chunk 0's headroom
        assert len(planted) - 8 <= D.HEADROOM
        desc = d[np.arange(3 * 64 + 37) % 64].copy()
        return buf, off, nbytes, desc, len(planted)
    return cached("bad", make)


def bad_forms(nbytes, planted_len, good_addr):
    return (("addr = umem_bytes + 1", nbytes + 1, planted_len),
            ("addr = umem_bytes - 8, len = 16", nbytes - 8, 16),
            ("len = 65536", good_addr, 65536),
            ("addr = 2^64 - 8, len = 16", (1 << 64) - 8, 16))


def test_bad_descriptors(ctx):
    """Each bad form at lane 0, at lane 63, at the last lane of the partial last tile, and a whole
    tile of them: status 255 and bit 0 there, the neighbours as the judges say."""
    keys = install(ctx, hfv.KEYSEL_ZERO)
    buf, off, nbytes, base, planted_len = bad_case()
    n = len(base)
    forms = bad_forms(nbytes, planted_len, int(base["addr"][5]))
    for name, addr, ln in forms:
        assert not D.desc_ok(addr, ln, nbytes)
    runs = [(name, {0: (a, w), 63: (a, w), n - 1: (a, w)}) for name, a, w in forms]
    runs.append(("a tile of them", {64 + j: forms[j % 4][1:] for j in range(64)}))
    for misalign in (0, 1):
        for name, where in runs:
            desc = base.copy()
            for i, (a, w) in where.items():
                desc["addr"][i], desc["len"][i] = a, w
            want, st = check(ctx, buf, off, nbytes, desc, [], keys, hfv.KEYSEL_ZERO, what=(name, misalign),
                             misalign=misalign)
            ok = hfv.bits_to_bool(want, n)
            bad = np.array(sorted(where))
            assert (st[bad] == D.BAD_DESC).all() and not ok[bad].any()
            assert (np.delete(st, bad) == 0).all() and np.delete(ok, bad).all()


# ---- 7. direction -------------------------------------------------------------------------------

@pytest.mark.parametrize("src", ["fuzz_br2_0", "fuzz_br3_1"])
def test_direction(ctx, src):
    """ifindex values from the BR's internal set and from outside it (the batch's own external
    interfaces, and two values no interface has); then the set cleared: every frame external."""
    keys = install(ctx, hfv.KEYSEL_ZERO)
    buf, off, nbytes, d = D.corpus(src, "permuted")
    desc = d.copy()
    desc["ifindex"][::7] = 0xFFFFFFFF
    desc["ifindex"][3::11] = 0
    iset = D.internal_set(src)
    assert 500 < np.isin(desc["ifindex"], iset).sum() < len(desc)
    with_set, st = check(ctx, buf, off, nbytes, desc, iset, keys, hfv.KEYSEL_ZERO, what="set")
    plain, st2 = check(ctx, buf, off, nbytes, desc, [], keys, hfv.KEYSEL_ZERO, what="empty set")
    assert np.array_equal(st, st2) and (with_set != plain).sum() >= 10


# ---- 8. repeats and overlaps --------------------------------------------------------------------

def test_repeated_and_overlapping_descriptors(ctx):
    """One frame named by 64 descriptors whose ifindex alternates between an external and an
    internal interface (a Cons = 0 frame: it passes by the ingress rule only), then descriptors whose
    bytes overlap."""
    keys = install(ctx, hfv.KEYSEL_ZERO)
    b = R.batch("br1", False)
    iset = R.internal_ifindices(b.cfg)
    idx = np.nonzero(b.sel_ext & b.forward & ~b.cons)[0][:2]
    buf, off, nbytes, desc = D.repeat_case(np.array(b.frames[idx]), np.array(b.lens[idx]), np.array(b.ifidx[idx]),
                                           iset[0])
    want, st = check(ctx, buf, off, nbytes, desc, iset, keys, hfv.KEYSEL_ZERO)
    ok = hfv.bits_to_bool(want, len(desc))
    assert ok[0:64:2].all() and not ok[1:64:2].any() and (st[:64] == 0).all()
    assert ok[64] and ok[65] and not ok[66] and st[66] != 0


# ---- 9. fail closed -----------------------------------------------------------------------------

def test_keysel_zero_without_key_fails_closed(ctx):
    ctx.key_add(0, K1)
    ctx.key_remove(0)
    buf, off, nbytes, desc = D.corpus("fuzz_br2_0", "packed")
    hk, _ = key1()
    want, st = check(ctx, buf, off, nbytes, desc, D.internal_set("fuzz_br2_0"), (hk, np.zeros(8, np.uint32)),
                     hfv.KEYSEL_ZERO, tag="no key")
    assert not want.any() and (st == 0).sum() > 2500


def test_keysel_ifid_with_a_slot_removed(ctx):
    """Interface 1's slot removed from the table: the frames that select it fail, the others pass."""
    hk, valid = install(ctx, hfv.KEYSEL_IFID)
    buf, off, nbytes, desc = D.corpus("fuzz_br1_1", "packed")
    full, _ = judges(ctx, buf, off, nbytes, desc, [], (hk, valid), hfv.KEYSEL_IFID, "keys")
    ctx.key_remove(1)
    part = valid.copy()
    part[0] &= np.uint32(~0x2 & 0xFFFFFFFF)
    want, st = check(ctx, buf, off, nbytes, desc, [], (hk, part), hfv.KEYSEL_IFID, tag="slot 1 removed")
    assert 100 < npass(want) < npass(full) - 100


# ---- status optional, timed form, arguments -----------------------------------------------------

def test_status_is_optional_and_timed_form(ctx):
    keys = install(ctx, hfv.KEYSEL_ZERO)
    buf, off, nbytes, desc = D.corpus("fuzz_br2_1", "inorder")
    iset = D.internal_set("fuzz_br2_1")
    want, _ = check(ctx, buf, off, nbytes, desc, iset, keys, hfv.KEYSEL_ZERO)
    got, st, _ = run_desc(ctx, buf, off, nbytes, desc, status=False)
    assert st is None and np.array_equal(got, want)
    got, st, ms = run_desc(ctx, buf, off, nbytes, desc, timed=True)
    assert 0.0 < ms < 100.0 and np.array_equal(got, want)
    # n == 0: 0.0, and nothing touched
    d, dd = to_device(buf[:8192]), dev_desc(desc[:8])
    bits, stt = fill_words(2), torch.full((8,), ST_FILL, dtype=torch.uint8, device=DEV)
    assert ctx.verify_frames_desc_timed(d, 8192, dd, 0, bits, status=stt) == 0.0
    torch.cuda.synchronize()
    assert (bits.cpu().numpy().view(np.uint64) == np.uint64(BITS_FILL)).all() and (stt == ST_FILL).all()


def test_arguments(ctx):
    buf, off, nbytes, desc = D.layout(*D.edge_source()[:2], "inorder")
    n = len(desc)
    d, dd = to_device(buf), dev_desc(desc)
    status = torch.full((n,), 0x77, dtype=torch.uint8, device=DEV)
    bits = torch.full((2,), 0x77, dtype=torch.int64, device=DEV)
    L, h = hfv.lib(), ctx._h
    ms = ctypes.c_float(-1.0)

    def both(umem_p, nbytes_, desc_p, n_, status_p, bits_p):
        a = L.hfv_verify_frames_desc(h, umem_p, nbytes_, desc_p, n_, status_p, bits_p, None)
        msg = L.hfv_last_error().decode()
        c = L.hfv_verify_frames_desc_timed(h, umem_p, nbytes_, desc_p, n_, status_p, bits_p, None, ctypes.byref(ms))
        assert a == c
        return a, msg

    u, p, s, w = d.data_ptr() + off, dd.data_ptr(), status.data_ptr(), bits.data_ptr()
    E = -errno.EINVAL
    for args, word in (((u, nbytes, None, n, s, w), "descriptor"), ((u, nbytes, p + 4, n, s, w), "8-byte"),
                       ((u, nbytes, p, n, s, None), "null"), ((u, nbytes, p, n, s, w + 4), "8-byte"),
                       ((None, nbytes, p, n, s, w), "null"), ((u, nbytes, p, (1 << 36) + 1, s, w), "2^36")):
        rc, msg = both(*args)
        assert rc == E and word in msg, (args, msg)
    assert L.hfv_verify_frames_desc(None, u, nbytes, p, n, s, w, None) == E
    assert L.hfv_verify_frames_desc_timed(h, u, nbytes, p, n, s, w, None, None) == E
    # n == 0: nothing to do, nothing written, even with null buffers
    assert both(None, 0, None, 0, None, None)[0] == 0 and ms.value == 0.0
    assert both(u, nbytes, p, 0, s, w)[0] == 0
    torch.cuda.synchronize()
    assert (status == 0x77).all() and (bits == 0x77).all()
    # a NULL umem of no bytes is no error: every descriptor but (0, 0) is invalid
    z = np.zeros(3, dtype=D.DTYPE)
    z["addr"], z["len"] = (0, 0, 1), (0, 1, 0)
    assert L.hfv_verify_frames_desc(h, None, 0, dev_desc(z).data_ptr(), 3, s, w, None) == 0
    torch.cuda.synchronize()
    assert status[:3].tolist() == [26, 255, 255] and int(bits[0]) == 0 and int(bits[1]) == 0x77


# ---- 10. stream order, key publication ----------------------------------------------------------

def test_stream_ordered(ctx):
    """H2D copies of the buffer and the descriptors (behind a few ms of other work), the call and a
    torch consumer of the bitmap on one non-default stream, one synchronize at the end."""
    keys = install(ctx, hfv.KEYSEL_ZERO)
    buf, off, nbytes, desc, iset = big_case()
    want, _ = judges(ctx, buf, off, nbytes, desc, iset, keys, hfv.KEYSEL_ZERO, "keys")
    n = len(desc)
    host = torch.from_numpy(np.array(buf, copy=True)).pin_memory()
    hdesc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).copy()).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.zeros(len(buf), dtype=torch.uint8, device=DEV)
        dd = torch.zeros(16 * n, dtype=torch.uint8, device=DEV)
        bits = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=DEV)
        torch.cuda._sleep(5_000_000)                         # the producer runs late
        d.copy_(host, non_blocking=True)
        dd.copy_(hdesc, non_blocking=True)
        ctx.verify_frames_desc(d.data_ptr() + off, nbytes, dd, n, bits, stream=s)
        out = bits.clone()                                   # the consumer
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want) and npass(want) > 5000


@BOTH
def test_key_publication(ctx, keysel):
    """Two calls on one stream held behind a sleep, a key_add of another key between them: each
    call's bitmap is the one of the key it was enqueued with (test_gpu_frames_fused.py's test, and
    test_gpu_key_publish.py's window, which is asserted open)."""
    from test_gpu_key_publish import Window
    buf, off, nbytes, desc = D.corpus("fuzz_br1_0", "permuted")
    n = len(desc)
    other = bytes(range(16))
    first = 0 if keysel == hfv.KEYSEL_ZERO else 1
    tables = []
    for key in (K1, other):
        raw = bytearray(ifid_raw())
        for ifid in range(first, 7):
            raw[16 * ifid:16 * ifid + 16] = key
        tables.append(bytes(raw))
    wants = [host_judge(buf, off, nbytes, desc, [], *orc.key_table(t), keysel)[0] for t in tables]
    assert npass(wants[0]) > 500 and not wants[1].any()
    ctx.set_keysel(keysel)
    ctx.key_add_batch(0, tables[0])
    d, dd = to_device(buf), dev_desc(desc)
    u = d.data_ptr() + off
    outs = [fill_words(65) for _ in range(3)]
    s = torch.cuda.Stream()
    ctx.verify_frames_desc(u, nbytes, dd, n, outs[2], stream=s)   # warm-up: table 0 is published
    w = Window(s)
    w.open()
    ctx.verify_frames_desc(u, nbytes, dd, n, outs[0], stream=s)
    w.mark()
    for ifid in range(first, 7):
        ctx.key_add(ifid, other)
    ctx.verify_frames_desc(u, nbytes, dd, n, outs[1], stream=s)
    w.assert_open()
    w.report("descriptor call, key publication")
    for o, want in zip(outs, (wants[0], wants[1], wants[0])):
        got = o.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:64], want) and got[64] == np.uint64(BITS_FILL)


# ---- 11. tile dealing ---------------------------------------------------------------------------

def run_deal(ctx, keysel, blocks, what):
    """deal_n frames as descriptors cycling over the 4001 packed frames of test_gpu_frames_fused's
    dealing batch (its host judge and its expected words: every full tile's word differs from its
    neighbours')."""
    frames, lens, passes = deal_case(keysel)
    buf, off, nbytes, base = cached(("deal buf", keysel), lambda: D.layout(frames, lens, "packed"))
    n = FD.deal_n(keysel, blocks)
    want = deal_expected(passes, n)
    desc = base[np.arange(n) % len(base)]
    d = cached(("deal dev", keysel), lambda: to_device(buf))
    dd = dev_desc(desc)
    words = (n + 63) // 64
    bits = fill_words(words + 1)
    st = torch.full((n + ST_GUARD,), ST_FILL, dtype=torch.uint8, device=DEV)
    ctx.verify_frames_desc(d.data_ptr() + off, nbytes, dd, n, bits, status=st)
    torch.cuda.synchronize()
    got = bits.cpu().numpy().view(np.uint64)
    assert got[words] == np.uint64(BITS_FILL), ("wrote past the bitmap", what)
    bad = np.nonzero(got[:words] != want)[0]
    assert not len(bad), (what, "%d bad words of %d, first %d: got %016x want %016x" % (
        len(bad), words, bad[0], int(got[bad[0]]), int(want[bad[0]])))
    assert int(got[words - 1]) >> 37 == 0
    assert (st[n:] == ST_FILL).all() and not (st[:n] == ST_FILL).any()


@BOTH
def test_tile_dealing_capped(request, ctx, cap, keysel):
    """1, 2 and 3 blocks: every wave claims five tiles or more, the block ranges are ragged and the
    last tile is partial (tests/fused_deal.py)."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    install(ctx, keysel)
    for blocks in FD.CAPS:
        cap(blocks)
        run_deal(ctx, keysel, blocks, (keysel, "cap %d" % blocks))


@BOTH
def test_tile_dealing_real_grid(ctx, keysel):
    """One block per CU, five tiles per wave and one over."""
    blocks = torch.cuda.get_device_properties(0).multi_processor_count
    install(ctx, keysel)
    run_deal(ctx, keysel, blocks, (keysel, "real grid of %d" % blocks))
