"""hfv_extract_records_rx / hfv_verify_frames_rx on the GPU: the direction-aware extract kernels
against the host counterpart (hfv_frame_extract per frame), the identity cases against
hfv_extract_records, the internal-interface set, the one-call path against the record oracle and
the router oracle, stream order, and argument checks.  Integer work: bit-exact."""
import ctypes
import errno

import numpy as np
import pytest

import br_topo as T
import frames_rx_ref as R
import orc
import scion_hfv as hfv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = hfv.VERDICT


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)                  # a fresh ctx: default record layout and keysel, no keys, empty set
    yield c
    c.synchronize()
    c.close()


def reslot(frames, slot):
    """The same frames in slots of `slot` bytes (longer frames are cut: len is clamped to slot)."""
    out = np.zeros((len(frames), slot), dtype=np.uint8)
    w = min(slot, frames.shape[1])
    out[:, :w] = frames[:, :w]
    return out


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def dev_lens(lens):
    return torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint16).view(np.int16).copy()).to(DEV)


def dev_ifx(ifidx):
    return torch.from_numpy(np.ascontiguousarray(ifidx, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def run_extract_rx(ctx, frames, lens, ifidx, n, layout=(40, 48, 64), fill=0xA5, extra=3, d_frames=None, rx=True):
    """extract_records_rx (or extract_records) over the first n frames into outputs that are
    pre-filled and `extra` entries longer than n.  Returns (status, records) of all n + extra
    entries and checks that the frames and the ifindex array are untouched."""
    inf_off, hf_off, stride = layout
    ctx.set_record_layout(inf_off, hf_off)
    slot = frames.shape[1]
    d = dev(frames) if d_frames is None else d_frames
    di = None if ifidx is None else dev_ifx(ifidx)
    recs = torch.full((n + extra, stride), fill, dtype=torch.uint8, device=DEV)
    status = torch.full((n + extra,), fill, dtype=torch.uint8, device=DEV)
    if rx:
        ctx.extract_records_rx(d, slot, dev_lens(lens), di, n, recs, status, stride=stride)
    else:
        ctx.extract_records(d, slot, dev_lens(lens), n, recs, status, stride=stride)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(frames.shape), frames), "frames were written"
    if di is not None:
        assert np.array_equal(di.cpu().numpy().view(np.uint32), np.asarray(ifidx, dtype=np.uint32)), "ifindex written"
    return status.cpu().numpy(), recs.cpu().numpy()


def check_extract_rx(ctx, frames, lens, ifidx, iset, n, layout=(40, 48, 64), d_frames=None):
    """The kernel against hfv_frame_extract per frame, membership computed here from ifidx and
    the set; entries past n keep their fill."""
    inf_off, hf_off, stride = layout
    ctx.set_internal_ifindices(iset)
    st, recs = run_extract_rx(ctx, frames, lens, ifidx, n, layout, d_frames=d_frames)
    internal = np.isin(ifidx[:n], iset)
    want_st, inf, hf = R.frame_extract(frames[:n], lens[:n], internal)
    assert np.array_equal(st[:n], want_st)
    assert np.array_equal(recs[:n, inf_off:inf_off + 8], inf)
    assert np.array_equal(recs[:n, hf_off:hf_off + 12], hf)
    bad = want_st != 0
    assert not recs[:n][bad][:, inf_off:inf_off + 8].any() and not recs[:n][bad][:, hf_off:hf_off + 12].any()
    assert (st[n:] == 0xA5).all() and (recs[n:] == 0xA5).all(), "wrote past n"
    return want_st, internal, inf


# ---- extract parity -----------------------------------------------------------------------------

@pytest.mark.parametrize("br,v6", [(b, v) for b in ("br2", "br3") for v in (False, True)], ids=R.IDS[2:])
def test_extract_rx_parity(ctx, br, v6):
    b = R.batch(br, v6)
    iset = R.internal_ifindices(b.cfg)
    st, internal, inf = check_extract_rx(ctx, b.frames, b.lens, b.ifidx, iset, 4096)
    folded = (inf != b.inf).any(axis=1)
    assert internal.sum() >= 1000 and folded.sum() >= 600          # the normalisation happened
    assert not folded[~internal].any() and not folded[b.cons].any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_extract_rx_counts(ctx, n):
    b = R.batch("br2", False)
    check_extract_rx(ctx, b.frames[:1025 + 3], b.lens, b.ifidx, R.internal_ifindices(b.cfg), n, (0, 8, 24))


@pytest.mark.parametrize("slot", [144, 256, 2048, 136])
def test_extract_rx_slots(ctx, slot):
    """144 is the loop's ring slot; 136 takes the kernel without 16-byte staging loads."""
    b = R.batch("br3", slot >= 144)                                 # IPv6 where its headers fit the slot
    st, internal, _ = check_extract_rx(ctx, reslot(b.frames, slot), b.lens, b.ifidx, R.internal_ifindices(b.cfg),
                                       4096, (0, 8, 24))
    assert (st == 0).sum() >= 1000 and (internal & (st == 0)).sum() >= 1000


def test_extract_rx_misaligned_frame_buffer(ctx):
    """A frame buffer that is 8- but not 16-byte aligned (the direct kernel)."""
    b = R.batch("br2", False)
    slot, n = 256, 1000
    fr = reslot(b.frames[:n], slot)
    buf = torch.zeros(n * slot + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[8:8 + n * slot]
    view.copy_(torch.from_numpy(fr.reshape(-1)))
    st, internal, _ = check_extract_rx(ctx, fr, b.lens, b.ifidx, R.internal_ifindices(b.cfg), n, (0, 8, 24),
                                       d_frames=view)
    assert (internal & (st == 0)).sum() >= 200


@pytest.mark.parametrize("layout", [(40, 48, 64), (0, 8, 24), (8, 16, 72)], ids=lambda x: "-".join(map(str, x)))
def test_extract_rx_layouts(ctx, layout):
    b = R.batch("br3", True)
    check_extract_rx(ctx, b.frames, b.lens, b.ifidx, R.internal_ifindices(b.cfg), 4096, layout)
    t = ctx.extract_records_rx_timed(dev(b.frames), b.frames.shape[1], dev_lens(b.lens), dev_ifx(b.ifidx), 4096,
                                     torch.zeros((4096, layout[2]), dtype=torch.uint8, device=DEV),
                                     torch.zeros(4096, dtype=torch.uint8, device=DEV), stride=layout[2])
    assert 0.0 < t < 100.0


# ---- identity cases -----------------------------------------------------------------------------

@pytest.mark.parametrize("slot", [2048, 136], ids=["staged", "direct"])
def test_extract_rx_identity_cases(ctx, slot):
    """An empty set, a NULL ifindex array and a set that holds none of the batch's ifindices: the
    outputs are byte for byte those of extract_records (all 64 record bytes, and past n)."""
    b = R.batch("br2", False)
    frames = reslot(b.frames, slot)
    n = 4001
    want = run_extract_rx(ctx, frames, b.lens, None, n, rx=False)
    iset = R.internal_ifindices(b.cfg)
    absent = [x for x in (100000, 77, 12, 65536 + 3) if x not in set(b.ifidx.tolist())]
    assert len(absent) >= 2
    for name, s, ifx in (("empty set", [], b.ifidx), ("null ifindex", iset, None), ("disjoint set", absent, b.ifidx)):
        ctx.set_internal_ifindices(s)
        got = run_extract_rx(ctx, frames, b.lens, ifx, n)
        assert np.array_equal(got[0], want[0]), name
        assert np.array_equal(got[1], want[1]), name
    ctx.set_internal_ifindices(iset)                                # and the set does change the records
    got = run_extract_rx(ctx, frames, b.lens, b.ifidx, n)
    assert np.array_equal(got[0], want[0]) and (got[1] != want[1]).any(axis=1).sum() >= 300


# ---- the set ------------------------------------------------------------------------------------

def test_internal_set_of_16_with_large_ifindices(ctx):
    b = R.batch("br2", False)
    n = 1025
    iset = [65536, 200, 70000, 2**32 - 1, 1 << 31, 65537, 300, 1000, 99999, 123456, 64, 4096, 250, 65535, 2**24, 31337]
    assert len(set(iset)) == 16
    rng = np.random.default_rng(7)
    others = np.array([1, 3, 63, 201, 65538, 2**32 - 2, 0], dtype=np.uint32)
    ifidx = np.where(rng.random(n) < 0.6, np.array(iset, dtype=np.uint32)[rng.integers(0, 16, n)],
                     others[rng.integers(0, len(others), n)]).astype(np.uint32)
    for x in iset:
        assert (ifidx == x).sum() >= 10, x                          # every entry selects some frames
    _, internal, inf = check_extract_rx(ctx, b.frames[:n], b.lens, ifidx, iset, n, (0, 8, 24))
    assert 400 < internal.sum() < 800 and (inf != b.inf[:n]).any(axis=1).sum() >= 100
    # a 17th entry: -EINVAL, and the old set still holds
    L = hfv.lib()
    arr17 = (ctypes.c_uint32 * 17)(*(iset + [5]))
    assert L.hfv_ctx_set_internal_ifindices(ctx._h, arr17, 17) == -errno.EINVAL
    assert L.hfv_ctx_set_internal_ifindices(ctx._h, None, 3) == -errno.EINVAL
    with pytest.raises(hfv.HfvError):
        ctx.set_internal_ifindices(iset + [5])
    st2, recs2 = run_extract_rx(ctx, b.frames[:n], b.lens, ifidx, n, (0, 8, 24))
    assert np.array_equal(recs2[:n, 0:8], inf)
    # cleared: identity again
    ctx.set_internal_ifindices([])
    st3, recs3 = run_extract_rx(ctx, b.frames[:n], b.lens, ifidx, n, (0, 8, 24))
    want = run_extract_rx(ctx, b.frames[:n], b.lens, None, n, (0, 8, 24), rx=False)
    assert np.array_equal(st3, want[0]) and np.array_equal(recs3, want[1])
    assert np.array_equal(recs3[:n, 0:8], b.inf[:n])


# ---- verify_frames_rx ---------------------------------------------------------------------------

def run_verify_frames_rx(ctx, frames, lens, ifidx, n, layout=(0, 8, 24), fill=-1, rx=True):
    inf_off, hf_off, stride = layout
    ctx.set_record_layout(inf_off, hf_off)
    recs = torch.zeros((n, stride), dtype=torch.uint8, device=DEV)
    status = torch.zeros(n, dtype=torch.uint8, device=DEV)
    words = (n + 63) // 64
    bits = torch.full((words + 1,), fill, dtype=torch.int64, device=DEV)
    if rx:
        ctx.verify_frames_rx(dev(frames), frames.shape[1], dev_lens(lens), dev_ifx(ifidx), n, recs, status, bits,
                             stride=stride)
    else:
        ctx.verify_frames(dev(frames), frames.shape[1], dev_lens(lens), n, recs, status, bits, stride=stride)
    torch.cuda.synchronize()
    w = bits.cpu().numpy().view(np.uint64)
    assert w[words] == np.uint64(fill & (2**64 - 1)), "wrote past the bitmap"
    return w[:words], status.cpu().numpy()


def record_oracle(b, n, hop_keys, valid, keysel):
    st, inf, hf = R.frame_extract(b.frames[:n], b.lens[:n], b.internal[:n])
    return R.oracle_bits(st, inf, hf, hop_keys, valid, keysel), st


@pytest.mark.parametrize("n", [4096, 4001])
def test_verify_frames_rx_vs_record_oracle_keysel_zero(ctx, n):
    b = R.batch("br2", False)
    ctx.key_add(0, T.KEYS[1])
    ctx.set_internal_ifindices(R.internal_ifindices(b.cfg))
    hk, valid = orc.key_table(T.KEYS[1])
    want, st = record_oracle(b, n, hk, valid, hfv.KEYSEL_ZERO)
    got, gst = run_verify_frames_rx(ctx, b.frames[:n], b.lens[:n], b.ifidx[:n], n)
    assert np.array_equal(gst, st)
    assert np.array_equal(got, want)
    npass = int(np.unpackbits(want.view(np.uint8)).sum())
    assert 500 < npass < (st == 0).sum()                    # both outcomes among the parsed frames
    if n % 64:
        assert got[-1] >> np.uint64(n % 64) == 0            # bits >= n


def test_verify_frames_rx_keysel_ifid_256_keys(ctx):
    b = R.batch("br3", True)
    raw = bytearray(orc.gen_key_table(256))
    for ifid in range(1, 7):                                 # the topology's AS interfaces: the AS key
        raw[16 * ifid:16 * ifid + 16] = T.KEYS[1]
    ctx.key_add_batch(0, bytes(raw))
    ctx.set_keysel(hfv.KEYSEL_IFID)
    ctx.set_internal_ifindices(R.internal_ifindices(b.cfg))
    hk, valid = orc.key_table(bytes(raw))
    want, st = record_oracle(b, 4096, hk, valid, hfv.KEYSEL_IFID)
    got, gst = run_verify_frames_rx(ctx, b.frames, b.lens, b.ifidx, 4096, layout=(40, 48, 64))
    assert np.array_equal(gst, st) and np.array_equal(got, want)
    assert int(np.unpackbits(want.view(np.uint8)).sum()) > 500


def test_verify_frames_rx_without_key_fails_closed(ctx):
    b = R.batch("br2", False)
    ctx.key_add(0, T.KEYS[1])
    ctx.key_remove(0)
    ctx.set_internal_ifindices(R.internal_ifindices(b.cfg))
    got, st = run_verify_frames_rx(ctx, b.frames, b.lens, b.ifidx, 4096)
    assert (st == 0).sum() > 3000 and not got.any()


@pytest.mark.parametrize("br,v6", R.CASES, ids=R.IDS)
def test_verify_frames_rx_vs_router_oracle(ctx, br, v6):
    """Frames whose verdict is decided by the hop-field check, received on an external interface
    or over the internal link towards an external one: the pass bit is the router oracle's
    SCION_FORWARD.  Plain verify_frames misjudges the internal link's frames."""
    b = R.batch(br, v6)
    R.check_selection_counts(b, br)
    ctx.key_add(0, T.KEYS[1])
    ctx.set_internal_ifindices(R.internal_ifindices(b.cfg))
    got, st = run_verify_frames_rx(ctx, b.frames, b.lens, b.ifidx, 4096)
    bits = hfv.bits_to_bool(got, 4096)
    assert (st[b.sel] == 0).all()
    assert np.array_equal(bits[b.sel], b.forward[b.sel])
    plain, _ = run_verify_frames_rx(ctx, b.frames, b.lens, b.ifidx, 4096, rx=False)
    pbits = hfv.bits_to_bool(plain, 4096)
    assert np.array_equal(pbits[b.sel_ext], b.forward[b.sel_ext])
    wrong = int((pbits[b.sel_int] != b.forward[b.sel_int]).sum())
    print(br, v6, "internal selected", int(b.sel_int.sum()), "verify_frames wrong on", wrong)
    if br in ("br2", "br3"):
        assert wrong >= 500, wrong


def test_verify_frames_rx_stream_ordered(ctx):
    """H2D copies of the frames, lengths and ifindices (behind a few ms of other work),
    verify_frames_rx and a torch consumer of the bitmap on one non-default stream, one synchronize
    at the end."""
    parts = [R.batch(br, False) for br in ("br2", "br3", "br2", "br3", "br2")]
    frames = np.concatenate([p.frames for p in parts])[:20000]
    lens = np.concatenate([p.lens for p in parts])[:20000]
    ifidx = np.concatenate([p.ifidx for p in parts])[:20000]
    n, slot = frames.shape
    iset = sorted(set(R.internal_ifindices(parts[0].cfg)) | set(R.internal_ifindices(parts[1].cfg)))
    internal = np.isin(ifidx, iset)                          # one set for the whole stream: the record oracle decides
    ctx.key_add(0, T.KEYS[1])
    ctx.set_record_layout(0, 8)
    ctx.set_internal_ifindices(iset)
    hk, valid = orc.key_table(T.KEYS[1])
    st, inf, hf = R.frame_extract(frames, lens, internal)
    want = R.oracle_bits(st, inf, hf, hk, valid, hfv.KEYSEL_ZERO)
    plain = R.oracle_bits(*R.frame_extract(frames, lens, False), hk, valid, hfv.KEYSEL_ZERO)
    assert (want != plain).sum() >= 100                      # the ifindex copy matters to the result
    host = torch.from_numpy(np.array(frames, copy=True)).pin_memory()
    hlens = torch.from_numpy(np.array(lens, copy=True).view(np.int16)).pin_memory()
    hifx = torch.from_numpy(np.array(ifidx, copy=True).view(np.int32)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.zeros((n, slot), dtype=torch.uint8, device=DEV)
        dl = torch.zeros(n, dtype=torch.int16, device=DEV)
        di = torch.zeros(n, dtype=torch.int32, device=DEV)
        recs = torch.empty((n, 24), dtype=torch.uint8, device=DEV)
        status = torch.empty(n, dtype=torch.uint8, device=DEV)
        bits = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=DEV)
        torch.cuda._sleep(5_000_000)                         # the producer runs late
        d.copy_(host, non_blocking=True)
        dl.copy_(hlens, non_blocking=True)
        di.copy_(hifx, non_blocking=True)
        ctx.verify_frames_rx(d, slot, dl, di, n, recs, status, bits, stream=s)
        out = bits.clone()                                   # the consumer
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


def test_frames_rx_arguments(ctx):
    b = R.batch("br2", False)
    n, slot = 64, b.frames.shape[1]
    d, dl, di = dev(b.frames[:n]), dev_lens(b.lens[:n]), dev_ifx(b.ifidx[:n])
    recs = torch.full((n + 1, 64), 0x77, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), 0x77, dtype=torch.uint8, device=DEV)
    bits = torch.full((1,), 0x77, dtype=torch.int64, device=DEV)
    L, h = hfv.lib(), ctx._h
    ctx.set_internal_ifindices(R.internal_ifindices(b.cfg))

    def both(frames_p, slot_, len_p, n_, recs_p, stride, status_p, bits_p):
        a = L.hfv_extract_records_rx(h, frames_p, slot_, len_p, di.data_ptr(), n_, recs_p, stride, status_p, None)
        c = L.hfv_verify_frames_rx(h, frames_p, slot_, len_p, di.data_ptr(), n_, recs_p, stride, status_p, bits_p,
                                   None)
        assert a == c
        return a

    p = dict(f=d.data_ptr(), l=dl.data_ptr(), r=recs.data_ptr(), s=status.data_ptr(), b=bits.data_ptr(),
             i=di.data_ptr())
    E = -errno.EINVAL
    assert both(p["f"], slot + 4, p["l"], n, p["r"], 64, p["s"], p["b"]) == E      # slot % 8
    assert both(p["f"], 56, p["l"], n, p["r"], 64, p["s"], p["b"]) == E            # slot < 64
    assert both(p["f"], slot, p["l"], n, p["r"] + 4, 64, p["s"], p["b"]) == E      # misaligned recs
    assert both(p["f"], slot, p["l"], n, p["r"], 60, p["s"], p["b"]) == E          # stride % 8
    assert both(p["f"], slot, p["l"], n, p["r"], 56, p["s"], p["b"]) == E          # HF@48 + 12 > 56
    assert both(None, slot, p["l"], n, p["r"], 64, p["s"], p["b"]) == E
    assert both(p["f"], slot, None, n, p["r"], 64, p["s"], p["b"]) == E
    assert both(p["f"], slot, p["l"], n, None, 64, p["s"], p["b"]) == E
    assert both(p["f"], slot, p["l"], n, p["r"], 64, None, p["b"]) == E
    assert L.hfv_verify_frames_rx(h, p["f"], slot, p["l"], p["i"], n, p["r"], 64, p["s"], None, None) == E
    assert L.hfv_verify_frames_rx(h, p["f"], slot, p["l"], p["i"], n, p["r"], 64, p["s"], p["b"] + 4, None) == E
    ms = ctypes.c_float(-1.0)
    assert L.hfv_extract_records_rx_timed(h, p["f"], slot, p["l"], p["i"], n, p["r"], 64, p["s"], None, None) == E
    assert L.hfv_extract_records_rx(None, p["f"], slot, p["l"], p["i"], n, p["r"], 64, p["s"], None) == E
    assert L.hfv_verify_frames_rx(None, p["f"], slot, p["l"], p["i"], n, p["r"], 64, p["s"], p["b"], None) == E
    ctx.set_record_layout(0, 8)
    assert both(p["f"], slot, p["l"], n, p["r"], 16, p["s"], p["b"]) == E          # HF@8 + 12 > 16
    # n == 0: nothing to do, nothing written, even with null buffers
    assert both(None, slot, None, 0, None, 24, None, None) == 0
    assert both(p["f"], slot, p["l"], 0, p["r"], 24, p["s"], p["b"]) == 0
    assert L.hfv_extract_records_rx_timed(h, p["f"], slot, p["l"], p["i"], 0, p["r"], 24, p["s"], None,
                                          ctypes.byref(ms)) == 0
    assert ms.value == 0.0
    torch.cuda.synchronize()
    assert (recs == 0x77).all() and (status == 0x77).all() and (bits == 0x77).all()
