"""The four *_timed entry points (hfv_verify_records_timed, hfv_verify_batches_timed,
hfv_extract_records_rx_timed, hfv_br_process_timed) against their plain forms: the same inputs
into separate outputs, bit-identical to each other and to the oracle, a positive kernel time, and
the argument rules the timed forms add (NULL kernel_ms, nothing to do).  4096 + 37 records or
frames: one full block of 64 tiles plus a ragged last tile.  Integer work: bit-exact."""
import ctypes
import errno
import functools

import numpy as np
import pytest

import br_fuzz as F
import br_topo as T
import frames_rx_ref as R
import orc
import scion_hfv as hfv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 4096 + 37
WORDS = (N + 63) // 64
EINVAL = -errno.EINVAL


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits_np(t):
    return host(t).view(np.uint64)


@functools.lru_cache(maxsize=None)
def record_case():
    """Key 0 of hf_single.npz, two runs of N generated records and the oracle's bitmaps."""
    g = orc.load_golden("hf_single.npz")
    key, hk, valid = g["raw_keys"][0].tobytes(), g["hop_keys"].reshape(-1), g["valid"]
    recs = [orc.gen_records(N, hk, 0, first_index=i * N) for i in range(2)]
    want = [orc.verify_records(r, hk, valid, 0) for r in recs]
    assert all(0 < int(np.unpackbits(w.view(np.uint8)).sum()) < N for w in want)   # both verdicts occur
    return key, recs, want


@functools.lru_cache(maxsize=None)
def frame_case():
    """N fuzz frames at BR 2 (external and internal links) with the router oracle's results and the
    host extract's records."""
    cfg = T.br_config("br2", False)
    frames, lens, ifidx = F.fuzz_batch(R.hop_inputs(False), "br2", False, N, seed=100, payload_max=1500)
    ref = frames.copy()
    oa, ov, oe, os_ = orc.br_process(ref, lens, ifidx, cfg, orc.hop_key(T.KEYS[1]))
    iset = R.internal_ifindices(cfg)
    st, inf, hf = R.frame_extract(frames, lens, np.isin(ifidx, iset))
    assert len(np.unique(ov)) >= 6 and (st == 0).sum() >= 1000 and (st != 0).any()
    return cfg, iset, frames, lens, ifidx, (ref, oa, ov, oe, os_), (st, inf, hf)


def frame_inputs(lens, ifidx):
    return (torch.from_numpy(lens.astype(np.uint16).view(np.int16)).to(DEV),
            torch.from_numpy(ifidx.astype(np.uint32).view(np.int32)).to(DEV))


def test_verify_records_timed(ctx):
    key, recs, want = record_case()
    ctx.key_add(0, key)
    d = dev(recs[0])
    plain, timed = (torch.full((WORDS,), -1, dtype=torch.int64, device=DEV) for _ in range(2))
    ctx.verify_records(d, N, plain)
    ms = ctx.verify_records_timed(d, N, timed)
    assert ms > 0
    assert np.array_equal(bits_np(plain), want[0]) and np.array_equal(bits_np(timed), want[0])
    L, h, out = hfv.lib(), ctx._h, ctypes.c_float(-1.0)
    assert L.hfv_verify_records_timed(h, d.data_ptr(), 64, N, timed.data_ptr(), None, None) == EINVAL
    assert L.hfv_verify_records_timed(h, d.data_ptr(), 64, 0, timed.data_ptr(), None, ctypes.byref(out)) == 0
    assert out.value == 0.0
    assert np.array_equal(bits_np(timed), want[0])       # neither call wrote


def test_verify_batches_timed(ctx):
    key, recs, want = record_case()
    ctx.key_add(0, key)
    d = [dev(r) for r in recs]

    def outputs():
        return [torch.full((WORDS,), -1, dtype=torch.int64, device=DEV) for _ in range(3)]

    def batch_list(bits):
        return ctx.service_batches([(d[0], N, bits[0]), (d[0], 0, bits[1]), (d[1], N, bits[2])])

    plain, timed = outputs(), outputs()
    ctx.verify_batches(batch_list(plain))
    ms = ctx.verify_batches_timed(batch_list(timed))
    assert ms > 0
    for got in (plain, timed):
        assert np.array_equal(bits_np(got[0]), want[0]) and np.array_equal(bits_np(got[2]), want[1])
        assert (host(got[1]) == -1).all()                # the empty batch writes nothing
    L, h, out = hfv.lib(), ctx._h, ctypes.c_float(-1.0)
    arr = batch_list(timed)
    assert L.hfv_verify_batches_timed(h, arr, len(arr), None, None) == EINVAL
    assert L.hfv_verify_batches_timed(h, arr, 0, None, ctypes.byref(out)) == 0 and out.value == 0.0
    out.value = -1.0
    empty = ctx.service_batches([(d[0], 0, timed[0]), (d[1], 0, timed[2])])
    assert L.hfv_verify_batches_timed(h, empty, len(empty), None, ctypes.byref(out)) == 0 and out.value == 0.0
    assert np.array_equal(bits_np(timed[0]), want[0]) and np.array_equal(bits_np(timed[2]), want[1])


def test_extract_records_rx_timed(ctx):
    cfg, iset, frames, lens, ifidx, _, (st, inf, hf) = frame_case()
    ctx.set_internal_ifindices(iset)
    slot = frames.shape[1]
    d, (dl, di) = dev(frames), frame_inputs(lens, ifidx)

    def outputs():
        return (torch.full((N, 64), 0xA5, dtype=torch.uint8, device=DEV),
                torch.full((N,), 0xA5, dtype=torch.uint8, device=DEV))

    (precs, pst), (trecs, tst) = outputs(), outputs()
    ctx.extract_records_rx(d, slot, dl, di, N, precs, pst, stride=64)
    ms = ctx.extract_records_rx_timed(d, slot, dl, di, N, trecs, tst, stride=64)
    assert ms > 0
    assert np.array_equal(host(precs), host(trecs)) and np.array_equal(host(pst), host(tst))
    got = host(trecs)
    assert np.array_equal(host(tst), st)
    assert np.array_equal(got[:, 40:48], inf) and np.array_equal(got[:, 48:60], hf)
    L, h, out = hfv.lib(), ctx._h, ctypes.c_float(-1.0)
    args = (d.data_ptr(), slot, dl.data_ptr(), di.data_ptr())
    assert L.hfv_extract_records_rx_timed(h, *args, N, trecs.data_ptr(), 64, tst.data_ptr(), None, None) == EINVAL
    assert L.hfv_extract_records_rx_timed(h, *args, 0, trecs.data_ptr(), 64, tst.data_ptr(), None,
                                          ctypes.byref(out)) == 0
    assert out.value == 0.0
    assert np.array_equal(host(trecs), got)              # neither call wrote


def test_br_process_timed(ctx):
    cfg, _, frames, lens, ifidx, (ref, oa, ov, oe, os_), _ = frame_case()
    ctx.br_set_config(cfg)
    ctx.key_add(0, T.KEYS[1])
    slot = frames.shape[1]
    dl, di = frame_inputs(lens, ifidx)

    def run(call):
        d = dev(frames)
        a, v = (torch.zeros(N, dtype=torch.uint8, device=DEV) for _ in range(2))
        e = torch.zeros(N, dtype=torch.int32, device=DEV)
        s = torch.zeros(hfv.BR_STATS_IFINDEX * 2 * hfv.BR_COUNTERS, dtype=torch.int64, device=DEV)
        ms = call(d, slot, dl, di, N, a, v, e, s)
        return ms, (d, a, v, e, s)

    _, plain = run(ctx.br_process)
    ms, timed = run(ctx.br_process_timed)
    assert ms > 0
    want = (ref, oa, ov, oe, os_.reshape(-1).view(np.int64))
    for got in (plain, timed):
        for g, w in zip(got, want):
            assert np.array_equal(host(g), w)
    L, h, out = hfv.lib(), ctx._h, ctypes.c_float(-1.0)
    d, a, v, e, s = timed
    args = (d.data_ptr(), slot, dl.data_ptr(), di.data_ptr())
    outs = (a.data_ptr(), v.data_ptr(), e.data_ptr(), s.data_ptr())
    assert L.hfv_br_process_timed(h, *args, N, *outs, None, None) == EINVAL
    assert L.hfv_br_process_timed(h, *args, 0, *outs, None, ctypes.byref(out)) == 0 and out.value == 0.0
    assert np.array_equal(host(d), ref) and np.array_equal(host(s), want[4])   # neither call wrote
