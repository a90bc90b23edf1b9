"""hfv_extract_records / hfv_verify_frames on the GPU: the extract kernel against the host parser
(hfv_frame_locate) plus a numpy gather, the one-call frames-to-bits path against the record
oracle and the router oracle, stream order, and argument checks.  Integer work: bit-exact."""
import ctypes
import errno

import numpy as np
import pytest

import br_fuzz as F
import br_topo as T
import orc
import scion_hfv as hfv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = hfv.VERDICT
MAC = lambda k, m: orc.cmac(m, k)   # noqa: E731  checker-side AES for building test paths
BRS = ("br1", "br2", "br3")


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)                  # a fresh ctx: default record layout and keysel, no keys
    yield c
    c.synchronize()
    c.close()


_CACHE = {}


def hop_inputs(v6):
    if ("hops", v6) not in _CACHE:
        brs = {b: T.OracleBR(T.br_config(b, v6)) for b in BRS}
        _CACHE[("hops", v6)] = F.hop_inputs(brs, v6, MAC)
    return _CACHE[("hops", v6)]


def fuzz(br, v6, n, seed):
    """A fuzz batch (frames, lens, ifindex), built once and left unchanged."""
    key = ("fuzz", br, v6, n, seed)
    if key not in _CACHE:
        b = F.fuzz_batch(hop_inputs(v6), br, v6, n, seed=seed, payload_max=1500)
        for a in b:
            a.setflags(write=False)
        _CACHE[key] = b
    return _CACHE[key]


def reslot(frames, slot):
    """The same frames in slots of `slot` bytes (longer frames are cut: len is clamped to slot)."""
    out = np.zeros((len(frames), slot), dtype=np.uint8)
    w = min(slot, frames.shape[1])
    out[:, :w] = frames[:, :w]
    return out


def host_extract(frames, lens, inf_off, hf_off, stride):
    """(status u8[n], records u8[n, stride]) by hfv_frame_locate per frame and a gather."""
    n, slot = frames.shape
    L = hfv.lib()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    status = np.zeros(n, dtype=np.uint8)
    io = np.zeros((n, 2), dtype=np.int64)
    base = frames.ctypes.data
    for i in range(n):
        status[i] = L.hfv_frame_locate(base + i * slot, min(int(lens[i]), slot), ctypes.byref(a), ctypes.byref(b))
        io[i] = a.value, b.value
    ok = np.nonzero(status == 0)[0]
    recs = np.zeros((n, stride), dtype=np.uint8)
    recs[ok[:, None], inf_off + np.arange(8)] = frames[ok[:, None], io[ok, 0:1] + np.arange(8)]
    recs[ok[:, None], hf_off + np.arange(12)] = frames[ok[:, None], io[ok, 1:2] + np.arange(12)]
    return status, recs


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def dev_lens(lens):
    return torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint16).view(np.int16).copy()).to(DEV)


def run_extract(ctx, frames, lens, n, layout=(40, 48, 64), fill=0xA5):
    """Extract on the GPU into pre-filled outputs; returns (status, records) as numpy and checks
    that the frames are untouched."""
    inf_off, hf_off, stride = layout
    ctx.set_record_layout(inf_off, hf_off)
    slot = frames.shape[1]
    d = dev(frames)
    recs = torch.full((max(n, 1), stride), fill, dtype=torch.uint8, device=DEV)
    status = torch.full((max(n, 1),), fill, dtype=torch.uint8, device=DEV)
    ctx.extract_records(d, slot, dev_lens(lens), n, recs, status, stride=stride)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), frames), "frames were written"
    return status.cpu().numpy(), recs.cpu().numpy()


def check_extract(ctx, frames, lens, n, layout=(40, 48, 64)):
    inf_off, hf_off, stride = layout
    frames = np.ascontiguousarray(frames[:max(n, 1)])
    st, recs = run_extract(ctx, frames, lens, n, layout)
    want_st, want = host_extract(frames[:n], lens[:n], inf_off, hf_off, stride)
    assert np.array_equal(st[:n], want_st)
    assert np.array_equal(recs[:n, inf_off:inf_off + 8], want[:, inf_off:inf_off + 8])
    assert np.array_equal(recs[:n, hf_off:hf_off + 12], want[:, hf_off:hf_off + 12])
    bad = want_st != 0
    assert not recs[:n][bad][:, inf_off:inf_off + 8].any() and not recs[:n][bad][:, hf_off:hf_off + 12].any()
    return want_st


@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_extract_fuzz_parity(ctx, v6):
    frames, lens, _ = fuzz("br1", v6, 20000, 300 + v6)
    st = check_extract(ctx, frames, lens, 20000)
    for s in (0, 17, 26, 34):
        assert (st == s).sum() >= 400, s


def test_extract_options_shift_and_long_paths(ctx):
    frames, lens, _, m = F.options_shift_batch(hop_inputs(False))
    st = check_extract(ctx, frames, lens, len(frames))
    assert (st == 0).all() and len(frames) == 11 * m
    for v6 in (False, True):
        frames, lens = T.to_slots([f for f, _ in F.long_path_frames(v6, MAC)])
        st = check_extract(ctx, frames, lens, len(frames))
        assert (st == 0).all()
        # cut one byte short of the hop field's end, which lies past the staged window: a parse error
        cut = np.array([hfv.frame_locate(bytes(frames[i, :lens[i]]))[2] + 11 for i in range(len(frames))], np.uint16)
        assert (cut > 256).all()
        st = check_extract(ctx, frames, cut, len(frames))
        assert (st == 17).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_extract_counts(ctx, n):
    frames, lens, _ = fuzz("br2", False, 1025, 310)
    st = check_extract(ctx, frames, lens, n)
    assert len(st) == n


def test_extract_leaves_records_past_n_alone(ctx):
    frames, lens, _ = fuzz("br2", False, 1025, 310)
    n = 65
    ctx.set_record_layout(0, 8)
    recs = torch.full((130, 24), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.full((130,), 0x5A, dtype=torch.uint8, device=DEV)
    ctx.extract_records(dev(frames[:130]), frames.shape[1], dev_lens(lens[:130]), n, recs, status)
    torch.cuda.synchronize()
    assert (recs[n:] == 0x5A).all() and (status[n:] == 0x5A).all()


@pytest.mark.parametrize("slot", [144, 256, 2048, 136, 64])
def test_extract_slots(ctx, slot):
    """144 is the loop's ring slot (frames straddle cache lines, lengths are clamped to it); 136
    and 64 take the kernel without 16-byte staging loads."""
    frames, lens, _ = fuzz("br1", slot >= 144, 4096, 320)    # IPv6 where its headers fit the slot
    st = check_extract(ctx, reslot(frames, slot), lens, 4096, (0, 8, 24))
    assert (st == 0).sum() >= (1000 if slot >= 136 else 0)   # slot 64 ends inside the SCION header


def test_extract_misaligned_frame_buffer(ctx):
    """A frame buffer that is 8- but not 16-byte aligned (the direct kernel)."""
    frames, lens, _ = fuzz("br1", False, 4096, 320)
    slot, n = 256, 1000
    fr = reslot(frames[:n], slot)
    ctx.set_record_layout(0, 8)
    buf = torch.zeros(n * slot + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[8:8 + n * slot]
    view.copy_(torch.from_numpy(fr.reshape(-1)))
    recs = torch.zeros((n, 24), dtype=torch.uint8, device=DEV)
    status = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ctx.extract_records(view, slot, dev_lens(lens[:n]), n, recs, status)
    torch.cuda.synchronize()
    want_st, want = host_extract(fr, lens[:n], 0, 8, 24)
    assert np.array_equal(status.cpu().numpy(), want_st)
    assert np.array_equal(recs.cpu().numpy()[:, :20], want[:, :20])


@pytest.mark.parametrize("layout", [(40, 48, 64), (0, 8, 24), (8, 16, 72)], ids=lambda x: "-".join(map(str, x)))
def test_extract_layouts(ctx, layout):
    frames, lens, _ = fuzz("br3", True, 4096, 330)
    check_extract(ctx, frames, lens, 4096, layout)
    t = ctx.extract_records_timed(dev(frames), frames.shape[1], dev_lens(lens), 4096,
                                  torch.zeros((4096, layout[2]), dtype=torch.uint8, device=DEV),
                                  torch.zeros(4096, dtype=torch.uint8, device=DEV), stride=layout[2])
    assert 0.0 < t < 100.0


# ---- verify_frames ----------------------------------------------------------------------------

def run_verify_frames(ctx, frames, lens, n, layout=(0, 8, 24), fill=-1):
    inf_off, hf_off, stride = layout
    ctx.set_record_layout(inf_off, hf_off)
    recs = torch.zeros((n, stride), dtype=torch.uint8, device=DEV)
    status = torch.zeros(n, dtype=torch.uint8, device=DEV)
    words = (n + 63) // 64
    bits = torch.full((words + 1,), fill, dtype=torch.int64, device=DEV)
    ctx.verify_frames(dev(frames), frames.shape[1], dev_lens(lens), n, recs, status, bits, stride=stride)
    torch.cuda.synchronize()
    b = bits.cpu().numpy().view(np.uint64)
    assert b[words] == np.uint64(fill & (2**64 - 1)), "wrote past the bitmap"
    return b[:words], status.cpu().numpy()


def oracle_bits(frames, lens, n, hop_keys, valid, keysel):
    """orc.verify_records over the host-extracted records (the oracle's 64-byte layout), ANDed
    with status == 0."""
    st, recs = host_extract(frames[:n], lens[:n], 40, 48, 64)
    bits = orc.verify_records(recs, hop_keys, valid, keysel)
    ok = np.zeros(len(bits) * 64, dtype=np.uint8)
    ok[:n] = st == 0
    return bits & np.packbits(ok, bitorder="little").view(np.uint64), st


@pytest.mark.parametrize("n", [4096, 4001])
def test_verify_frames_vs_record_oracle_keysel_zero(ctx, n):
    frames, lens, _ = fuzz("br1", False, 4096, 340)
    ctx.key_add(0, T.KEYS[1])
    hk, valid = orc.key_table(T.KEYS[1])
    want, st = oracle_bits(frames, lens, n, hk, valid, hfv.KEYSEL_ZERO)
    got, gst = run_verify_frames(ctx, frames[:n], lens[:n], n)
    assert np.array_equal(gst, st)
    assert np.array_equal(got, want)
    npass = int(np.unpackbits(want.view(np.uint8)).sum())
    assert 500 < npass < (st == 0).sum()                    # both outcomes among the parsed frames
    if n % 64:
        assert got[-1] >> np.uint64(n % 64) == 0            # bits >= n


def test_verify_frames_keysel_ifid_256_keys(ctx):
    frames, lens, _ = fuzz("br1", True, 4096, 341)
    raw = bytearray(orc.gen_key_table(256))
    for ifid in range(1, 7):                                 # the topology's AS interfaces: the AS key
        raw[16 * ifid:16 * ifid + 16] = T.KEYS[1]
    ctx.key_add_batch(0, bytes(raw))
    ctx.set_keysel(hfv.KEYSEL_IFID)
    hk, valid = orc.key_table(bytes(raw))
    want, st = oracle_bits(frames, lens, 4096, hk, valid, hfv.KEYSEL_IFID)
    got, gst = run_verify_frames(ctx, frames, lens, 4096, layout=(40, 48, 64))
    assert np.array_equal(gst, st) and np.array_equal(got, want)
    assert int(np.unpackbits(want.view(np.uint8)).sum()) > 500


def test_verify_frames_without_key_fails_closed(ctx):
    frames, lens, _ = fuzz("br1", False, 4096, 340)
    ctx.key_add(0, T.KEYS[1])
    ctx.key_remove(0)
    got, st = run_verify_frames(ctx, frames, lens, 4096)
    assert (st == 0).sum() > 3000 and not got.any()


@pytest.mark.parametrize("br,v6", [(b, v) for b in ("br1", "br2") for v in (False, True)],
                         ids=lambda x: x if isinstance(x, str) else ("ipv6" if x else "ipv4"))
def test_verify_frames_vs_router_oracle(ctx, br, v6):
    """Frames that reach the router on an external interface and whose verdict is decided by the
    hop-field check: the pass bit is the router oracle's SCION_FORWARD."""
    frames, lens, ifidx = fuzz(br, v6, 4096, 100 + v6)       # the batches of test_frames_host.py
    cfg = T.br_config(br, v6)
    _, verdict, _, _ = orc.br_process(frames.copy(), lens, ifidx, cfg, orc.hop_key(T.KEYS[1]))
    internal = [cfg.int_ifaces[i].ifindex for i in range(cfg.n_int_ifaces)]
    sel = ~np.isin(ifidx, internal) & np.isin(verdict, [V["SCION_FORWARD"], V["INVALID_HF"]])
    assert sel.sum() >= 1000 and (verdict[sel] == V["INVALID_HF"]).sum() >= 40
    ctx.key_add(0, T.KEYS[1])
    got, st = run_verify_frames(ctx, frames, lens, 4096)
    bits = hfv.bits_to_bool(got, 4096)
    assert (st[sel] == 0).all()
    assert np.array_equal(bits[sel], verdict[sel] == V["SCION_FORWARD"])


def test_verify_frames_stream_ordered(ctx):
    """H2D copy of the frames (behind a few ms of other work), verify_frames and a torch consumer
    of the bitmap on one non-default stream, one synchronize at the end."""
    frames, lens, _ = fuzz("br1", False, 20000, 300)
    n, slot = frames.shape
    ctx.key_add(0, T.KEYS[1])
    ctx.set_record_layout(0, 8)
    hk, valid = orc.key_table(T.KEYS[1])
    want, _ = oracle_bits(frames, lens, n, hk, valid, hfv.KEYSEL_ZERO)
    host = torch.from_numpy(np.array(frames, copy=True)).pin_memory()
    hlens = torch.from_numpy(np.array(lens, copy=True).view(np.int16)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.zeros((n, slot), dtype=torch.uint8, device=DEV)
        dl = torch.zeros(n, dtype=torch.int16, device=DEV)
        recs = torch.empty((n, 24), dtype=torch.uint8, device=DEV)
        status = torch.empty(n, dtype=torch.uint8, device=DEV)
        bits = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=DEV)
        torch.cuda._sleep(5_000_000)                         # the producer runs late
        d.copy_(host, non_blocking=True)
        dl.copy_(hlens, non_blocking=True)
        ctx.verify_frames(d, slot, dl, n, recs, status, bits, stream=s)
        out = bits.clone()                                   # the consumer
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


def test_frames_arguments(ctx):
    frames, lens, _ = fuzz("br2", False, 1025, 310)
    n, slot = 64, frames.shape[1]
    d, dl = dev(frames[:n]), dev_lens(lens[:n])
    recs = torch.full((n + 1, 64), 0x77, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), 0x77, dtype=torch.uint8, device=DEV)
    bits = torch.full((1,), 0x77, dtype=torch.int64, device=DEV)
    L, h = hfv.lib(), ctx._h

    def both(frames_p, slot_, len_p, n_, recs_p, stride, status_p, bits_p):
        a = L.hfv_extract_records(h, frames_p, slot_, len_p, n_, recs_p, stride, status_p, None)
        b = L.hfv_verify_frames(h, frames_p, slot_, len_p, n_, recs_p, stride, status_p, bits_p, None)
        assert a == b
        return a

    p = dict(f=d.data_ptr(), l=dl.data_ptr(), r=recs.data_ptr(), s=status.data_ptr(), b=bits.data_ptr())
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
    assert L.hfv_verify_frames(h, p["f"], slot, p["l"], n, p["r"], 64, p["s"], None, None) == E
    assert L.hfv_verify_frames(h, p["f"], slot, p["l"], n, p["r"], 64, p["s"], p["b"] + 4, None) == E
    ms = ctypes.c_float(-1.0)
    assert L.hfv_extract_records_timed(h, p["f"], slot, p["l"], n, p["r"], 64, p["s"], None, None) == E
    assert L.hfv_extract_records(None, p["f"], slot, p["l"], n, p["r"], 64, p["s"], None) == E
    ctx.set_record_layout(0, 8)
    assert both(p["f"], slot, p["l"], n, p["r"], 16, p["s"], p["b"]) == E          # HF@8 + 12 > 16
    # n == 0: nothing to do, nothing written, even with null buffers
    assert both(None, slot, None, 0, None, 24, None, None) == 0
    assert both(p["f"], slot, p["l"], 0, p["r"], 24, p["s"], p["b"]) == 0
    assert L.hfv_extract_records_timed(h, p["f"], slot, p["l"], 0, p["r"], 24, p["s"], None, ctypes.byref(ms)) == 0
    assert ms.value == 0.0
    torch.cuda.synchronize()
    assert (recs == 0x77).all() and (status == 0x77).all() and (bits == 0x77).all()
