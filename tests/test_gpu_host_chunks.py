"""The chunk pipelines of hfv_verify_records_host and hfv_br_process_host on the GPU, at chunks of 64,
100 and 128 (test hooks), so that a few hundred records or frames cross every chunk edge, reuse both
stream slots and fill several retry rounds; the model, the corpora and the asserted table are those of
tests/host_chunks.py, which tests/test_host_chunks.py holds on the CPU.

Every case has two judges: the rule (hf_bits / key_tables for records, the oracle router on the whole
frames for the router) and the device entry point (hfv_verify_records, hfv_br_process) on a device copy
of the same input.  hfv_debug_host_chunk_counts must report exactly what the model says the call ran.
Every output lies between guards and is pre-filled with a value no result can take; the inputs are
compared unchanged afterwards.  Integer work: every comparison is exact.

Every test uses test hooks and runs in a child process on lib/libscionhfv_test.so
(conftest.rerun_on_test_build), and restores the hooks in a `finally`.

`make hostchunk` builds five libraries with one wrong step each (csrc/hfv_host_path.cpp; number 1 in the
schedule itself, csrc/hfv_host_pipe.h); this module must fail on every one, by assertions alone: run it
with HFV_LIB=lib/libscionhfv_hostchunkN.so HFV_TEST_BUILD_CHILD=1.  What fails (of the 13 cases; every
failure is an assertion):
  hostchunk1  a retired chunk's results to the place of the chunk on the other slot: all 13.  The 9
              record cases (test_records_*, both test_records_every_chunk_edge, test_three_host_threads,
              test_records_router_records_on_one_ctx): word 0 keeps its pre-fill.  The 6 router cases
              (both test_router_every_row, test_router_window_grows_and_shrinks, test_router_ipv6_tables,
              test_three_host_threads, test_records_router_records_on_one_ctx): from two chunks on,
              frames keep their pre-fill or carry another chunk's results.  (The router's copy of this
              step was hostchunk4 while the two paths had a loop each; that number is retired.)
  hostchunk2  a ragged chunk's floor(cnt / 64) words: the 9 record cases but
              test_records_chunk_sizes_back_to_back (6656 records: no ragged chunk); first at n = 63,
              whose only word keeps its pre-fill
  hostchunk3  later chunks gathered at first * 24: the same 9; the second chunk's words are those of
              other records (the compact layout, stride 24, cannot tell: the wider ones fail)
  hostchunk5  the counters zeroed before every chunk: the 6 router cases, by the counters alone (every
              frame result is right), from the first row with a retry round on
  hostchunk6  a retry round scattered backwards: the same 6; the retried frames carry each other's
              results (one retried frame, n = 1, cannot tell)"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import br_fuzz as F
import br_topo as T
import frames_rx_ref as R
import hf_bits as HB
import host_chunks as HC
import key_tables as KT
import orc
import scion_hfv as hfv
from conftest import ROOT, rerun_on_test_build
from test_gpu_hf_bits import FILL, DevBits, HostBits, dev, install

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

A_FILL = V_FILL = 0xEE             # no action (0..4, 0xff inside the library) and no verdict
E_FILL = 0x5A5A5A5A                # no ifindex
ROW_FILL = 0xA5
G = 64                             # guard entries on either side of action, verdict and egress
SLOT = HC.SLOT
STATS_PATTERN = (np.arange(64 * 2 * 11, dtype=np.uint64) * np.uint64(0x9E37) + np.uint64(12345)).reshape(64, 2, 11)


@contextlib.contextmanager
def fresh_ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    try:
        yield c
        c.synchronize()
    finally:
        c.close()


def reset_hooks():
    hfv.Ctx.debug_records_host_chunk(0)
    hfv.Ctx.debug_br_host_chunk(0)
    hfv.Ctx.debug_host_inline_rows(0)


# ---- hfv_verify_records_host -------------------------------------------------------------------

def host_records(ctx, recs, n, stride, want, what, chunk):
    """One call over an exact-size pageable copy of recs[:n]: the rule, the guards, the inputs, and
    the counts against the model (chunk None: the zero-copy path, no chunks).  Returns the words."""
    src = np.array(recs[:n], copy=True)
    keep = src.copy()
    o = HostBits(n)
    ctx.verify_records_host(src, n, o.bits, stride=stride)
    got = hfv.Ctx.debug_host_chunk_counts()
    assert np.array_equal(src, keep), ("records were written", what)
    o.check(want[:n], what)
    assert got == HC.counts(n, chunk), ("counts", what, n, chunk, got)
    return o.bits.copy()


def device_records(ctx, recs, n, stride, want, what):
    o = DevBits(n)
    ctx.verify_records(dev(recs[:n]), n, o.bits, stride=stride)
    o.check(want[:n], ("device", what))
    return o.bits.cpu().numpy().view(np.uint64)


def records_legs(ctx, keysel, layouts, chunks, inlines):
    install(ctx)
    ctx.set_keysel(keysel)
    for layout in layouts:
        ctx.set_record_layout(layout[0], layout[1])
        recs, passes, _ = HC.hf_dealt(keysel, layout)
        judge = {}
        for chunk in chunks:
            hfv.Ctx.debug_records_host_chunk(chunk)
            for inline in inlines:
                hfv.Ctx.debug_host_inline_rows(inline)
                for n in HC.rec_sizes(len(recs), chunk):
                    what = (keysel, layout, chunk, inline, n)
                    if n not in judge:
                        judge[n] = device_records(ctx, recs, n, layout[2], passes, what)
                    got = host_records(ctx, recs, n, layout[2], passes, what, chunk)
                    assert np.array_equal(got, judge[n]), what
                    assert HC.counts(n, chunk)[3] == max(0, -(-n // chunk) - 2)
    assert HC.counts(3 * 64, 64)[3] == 1 and HC.counts(2 * 64, 64)[3] == 0      # reuses from three chunks on


@pytest.mark.parametrize("keysel", [0, 1])
def test_records_every_chunk_edge(request, keysel):
    """Both chunk sizes, three layouts, n on every side of a chunk edge, the staging copies inline and
    (16 rows) through the host pool's partition."""
    if rerun_on_test_build(request):
        return
    with fresh_ctx() as ctx:
        try:
            records_legs(ctx, keysel, HB.LAYOUTS, HC.REC_CHUNKS, (0, 16))
        finally:
            reset_hooks()


def test_three_host_threads(request):
    """HFV_HOST_THREADS=3 (read once per process: a fresh one): 100-row and 37-row chunks cut in
    three, n * k / 3, for the record gather and the router's window copies."""
    if rerun_on_test_build(request):
        return
    if os.environ.get("HFV_HOST_THREADS") != "3":
        env = dict(os.environ, HFV_HOST_THREADS="3")
        r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m",
                            "gpu or not gpu", request.node.nodeid], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0 and " passed" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])
        return
    with fresh_ctx() as ctx:
        try:
            records_legs(ctx, 1, (HB.LAYOUTS[2],), HC.REC_CHUNKS, (16,))
            router_setup(ctx)
            for row in (("mix", HC.MIX_N, 100, 64), ("mix", HC.MIX_N, 128, 136), ("r127", 385, 128, 64)):
                hfv.Ctx.debug_host_inline_rows(16)
                router_row(ctx, *row)
        finally:
            reset_hooks()


def test_records_partial_table_and_empty_slot_0(request):
    """KEYSEL_IFID with the even slots only: every chunk's launch, on either stream, sees the same
    published table.  KEYSEL_ZERO with slot 0 empty: every word 0."""
    if rerun_on_test_build(request):
        return
    layout = HB.LAYOUTS[0]
    try:
        with fresh_ctx() as ctx:
            install(ctx, range(0, 256, 2))
            ctx.set_keysel(1)
            recs, _, partial = HC.hf_dealt(1, layout)
            for chunk in HC.REC_CHUNKS:
                hfv.Ctx.debug_records_host_chunk(chunk)
                for n in (len(recs), 3 * chunk + 37):
                    got = host_records(ctx, recs, n, 64, partial, ("partial", chunk, n), chunk)
                    assert np.array_equal(got, device_records(ctx, recs, n, 64, partial, ("partial", chunk, n)))
        with fresh_ctx() as ctx:
            install(ctx, range(1, 256))
            recs, passes, _ = HC.hf_dealt(0, layout)
            none = np.zeros(len(recs), dtype=bool)
            for chunk in HC.REC_CHUNKS:
                hfv.Ctx.debug_records_host_chunk(chunk)
                for n in (len(recs), 2 * chunk + 1):
                    assert not host_records(ctx, recs, n, 64, none, ("no key 0", chunk, n), chunk).any()
            ctx.key_add(0, HB.raw_keys()[:16])
            host_records(ctx, recs, len(recs), 64, passes, "key 0 added", 128)
    finally:
        reset_hooks()


@pytest.mark.parametrize("between", [False, True], ids=["host-calls-only", "user-stream-launch-between"])
def test_records_key_change_between_calls(request, between):
    """Tables A, B, A installed between three calls at chunk 64 (71 chunks each): every chunk of a call
    shows that call's table; in every chunk the three tables' words differ (host_chunks.kt_roll_ok).
    Then the same with a hfv_verify_records launch on a user stream between the calls, which leaves
    that stream a reader of the table the next install must not overwrite early."""
    if rerun_on_test_build(request):
        return
    recs, want = HC.kt_rolled()
    n = len(recs)
    try:
        with fresh_ctx() as ctx:
            ctx.set_keysel(1)
            hfv.Ctx.debug_records_host_chunk(64)
            d, s = dev(recs), torch.cuda.Stream()
            torch.cuda.synchronize()
            for name in ("A", "B", "A", "C"):
                ctx.key_add_batch(0, KT.tables()[name][0])
                got = host_records(ctx, recs, n, 64, want[name], ("table", name), 64)
                for c, _, first, cnt, words in HC.schedule(n, 64):
                    assert np.array_equal(got[first // 64:first // 64 + words],
                                          HB.bitmap(want[name][first:first + cnt])), ("chunk", c, "table", name)
                if between:
                    o = DevBits(n)
                    ctx.verify_records(d, n, o.bits, stream=s)
                    s.synchronize()
                    o.check(want[name], ("user stream", name))
    finally:
        reset_hooks()


def test_records_registered_ring_takes_no_chunks(request):
    if rerun_on_test_build(request):
        return
    layout = HB.LAYOUTS[0]
    recs, passes, _ = HC.hf_dealt(0, layout)
    ring = hfv.host_array((3 * 128 + 37, 64), np.uint8)
    try:
        with fresh_ctx() as ctx:
            install(ctx)
            ctx.host_register(ring)
            try:
                for chunk in HC.REC_CHUNKS:
                    hfv.Ctx.debug_records_host_chunk(chunk)
                    host_records(ctx, recs, 3 * chunk + 37, 64, passes, "pageable first", chunk)   # counts not 0
                    for n in HC.rec_sizes(len(ring), chunk)[1:]:
                        ring[:n] = recs[:n]
                        o = HostBits(n)
                        ctx.verify_records_host(ring, n, o.bits, stride=64)
                        o.check(passes[:n], ("ring", chunk, n))
                        assert hfv.Ctx.debug_host_chunk_counts() == (0, 0, 0, 0), (chunk, n)
            finally:
                ctx.host_unregister(ring)
    finally:
        reset_hooks()


def test_records_chunk_sizes_back_to_back(request):
    """Chunk 64, the default chunk, chunk 128 on one ctx: the staging is allocated once, at its full
    size, whatever the chunk."""
    if rerun_on_test_build(request):
        return
    layout = HB.LAYOUTS[2]
    recs, passes, _ = HC.hf_dealt(1, layout)
    n = len(recs)
    try:
        with fresh_ctx() as ctx:
            install(ctx)
            ctx.set_keysel(1)
            ctx.set_record_layout(layout[0], layout[1])
            got = []
            for chunk in (64, 0, 128):
                hfv.Ctx.debug_records_host_chunk(chunk)
                got.append(host_records(ctx, recs, n, layout[2], passes, ("back to back", chunk),
                                        chunk or HC.REC_CHUNK_DEFAULT))
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    finally:
        reset_hooks()


# ---- hfv_br_process_host -----------------------------------------------------------------------

_JUDGE = {}


def router_setup(ctx, v6=False):
    ctx.br_set_config(T.br_config("br1", v6))
    ctx.key_add(0, T.KEYS[1])


def device_router(ctx, key, frames, lens, ifidx):
    """hfv_br_process on a device copy of the whole frames: (action, verdict, egress, stats, frames)."""
    if key not in _JUDGE:
        n, slot = frames.shape
        d = dev(frames)
        a = torch.zeros(n, dtype=torch.uint8, device="cuda")
        v = torch.zeros_like(a)
        e = torch.zeros(n, dtype=torch.int32, device="cuda")
        s = torch.zeros(64 * 2 * 11, dtype=torch.int64, device="cuda")
        ctx.br_process(d, slot, dev(lens.view(np.int16)), dev(ifidx.view(np.int32)), n, a, v, e, s)
        torch.cuda.synchronize()
        _JUDGE[key] = (a.cpu().numpy(), v.cpu().numpy(), e.cpu().numpy(),
                       s.cpu().numpy().view(np.uint64).reshape(64, 2, 11), d.cpu().numpy())
    return _JUDGE[key]


def host_router(ctx, frames, lens, ifidx, window, want, what, stats=True, calls=2):
    """`calls` calls on the same arrays (the frames put back in between): every call's results and
    rewritten frames equal `want` (action, verdict, egress, stats, frames), the guards and the inputs
    stand, and the counters are added to what `stats` held.  Returns the counts of the last call."""
    n, slot = frames.shape
    wa, wv, we, ws, wout = want
    buf = np.full((n + 1, slot), ROW_FILL, np.uint8)
    a = np.full(n + 2 * G, A_FILL, np.uint8)
    v = np.full(n + 2 * G, V_FILL, np.uint8)
    e = np.full(n + 2 * G, E_FILL, np.int32)
    ln, ix = np.array(lens, copy=True), np.array(ifidx, copy=True)
    st = STATS_PATTERN.copy() if stats else None
    for call in range(1, calls + 1):
        buf[:n] = frames
        a[:], v[:], e[:] = A_FILL, V_FILL, E_FILL
        ctx.br_process_host(buf[:n], slot, ln, ix, n, a[G:G + n], v[G:G + n], e[G:G + n], st, window=window)
        got = hfv.Ctx.debug_host_chunk_counts()
        assert np.array_equal(ln, lens) and np.array_equal(ix, ifidx), ("inputs were written", what)
        assert (buf[n] == ROW_FILL).all(), ("the row after the last frame was written", what)
        for arr, fill, name in ((a, A_FILL, "action"), (v, V_FILL, "verdict"), (e, E_FILL, "egress")):
            assert (arr[:G] == fill).all() and (arr[G + n:] == fill).all(), ("wrote outside " + name, what)
        bad = np.nonzero((a[G:G + n] != wa) | (v[G:G + n] != wv) | (e[G:G + n] != we) | (buf[:n] != wout).any(axis=1))[0]
        assert not len(bad), (what, "call %d: %d frames differ, first %d: got (%d,%d,%d) want (%d,%d,%d)" % (
            call, len(bad), bad[0], a[G + bad[0]], v[G + bad[0]], e[G + bad[0]], wa[bad[0]], wv[bad[0]], we[bad[0]]))
        if stats:
            with np.errstate(over="ignore"):
                assert np.array_equal(st, STATS_PATTERN + np.uint64(call) * ws), ("counters", what, "call %d" % call)
    return got


def router_row(ctx, name, n, chunk, window, **kw):
    """One row of the asserted table: the oracle on the whole frames, hfv_br_process on a device copy
    bit for bit, and the counts the table says."""
    frames, lens, ifidx = HC.corpus_prefix(name, n)
    want = HC.oracle(name, n)
    judge = device_router(ctx, (name, n), frames, lens, ifidx)
    orc.assert_br_equal(judge[:4], judge[4], want[:4], want[4], "hfv_br_process against the oracle")
    hfv.Ctx.debug_br_host_chunk(chunk)
    got = host_router(ctx, frames, lens, ifidx, window, want, (name, n, chunk, window), **kw)
    chunks, reuses, per_chunk, rounds = HC.TABLE[(name, n, chunk, window)]
    assert got == (chunks, rounds, sum(per_chunk), reuses), ("counts", name, n, chunk, window, got)
    return got


@pytest.mark.parametrize("chunk", [128, 100])
def test_router_every_row(request, chunk):
    """Every row of host_chunks.TABLE at this chunk: every size on every side of a chunk edge, every
    window, the retried totals cap - 1 (odd), cap, cap + 1 and 2 * cap."""
    if rerun_on_test_build(request):
        return
    rows = [r for r in HC.TABLE if r[2] == chunk]
    assert len(rows) == {128: 62, 100: 6}[chunk]
    try:
        with fresh_ctx() as ctx:
            router_setup(ctx)
            for row in rows:
                router_row(ctx, *row)
            if chunk == 128:
                # two full rounds and then frames that are not retried: the loop's empty round adds none
                assert router_row(ctx, "r256", 385, 128, 64, calls=1)[1:3] == (2, 256)
    finally:
        reset_hooks()


def test_router_window_grows_and_shrinks(request):
    """Window 64, slot, 128, 64 on one ctx: the window buffers grow once and later calls use a
    smaller pitch in the larger buffer; then without counters, and one frame."""
    if rerun_on_test_build(request):
        return
    try:
        with fresh_ctx() as ctx:
            router_setup(ctx)
            for window in (64, SLOT, 128, 64):
                router_row(ctx, "mix", 385, 128, window)
            router_row(ctx, "mix", HC.MIX_N, 128, 64, stats=False)
            router_row(ctx, "mix", 385, 128, 256, stats=False, calls=1)
            for window in (64, SLOT):
                router_row(ctx, "mix", 1, 128, window)
    finally:
        reset_hooks()


def test_records_router_records_on_one_ctx(request):
    """The two host paths share the ctx's two host streams: a records call, a router call and a
    records call again, slot 0's key changed in between (the router's key, then the corpus' own)."""
    if rerun_on_test_build(request):
        return
    layout = HB.LAYOUTS[0]
    recs, passes, _ = HC.hf_dealt(1, layout)
    n = 3 * 64 + 37
    try:
        with fresh_ctx() as ctx:
            install(ctx)
            ctx.set_keysel(1)
            ctx.br_set_config(T.br_config("br1"))
            hfv.Ctx.debug_records_host_chunk(64)
            first = host_records(ctx, recs, n, 64, passes, "before the router call", 64)
            ctx.key_add(0, T.KEYS[1])
            router_row(ctx, "mix", 385, 128, 64)
            ctx.key_add(0, HB.raw_keys()[:16])
            again = host_records(ctx, recs, n, 64, passes, "after the router call", 64)
            assert np.array_equal(first, again)
            ctx.key_add(0, T.KEYS[1])
            router_row(ctx, "mix", HC.MIX_N, 128, 136)
    finally:
        reset_hooks()


def test_router_ipv6_tables(request):
    """The IPv6 tables on 300 IPv6 fuzz frames at chunk 128, window 128: three chunks, one slot
    reused, two retry rounds.  The retried count lies between the frames the rule calls retried and
    those plus the ones it leaves open (host_chunks.retried_rule)."""
    if rerun_on_test_build(request):
        return
    n = 300
    frames, lens, ifidx = F.fuzz_batch(R.hop_inputs(True), "br1", True, n, 61, slot=SLOT, payload_max=600)
    out = frames.copy()
    oa, ov, oe, os_ = orc.br_process(out, lens, ifidx, T.br_config("br1", True), orc.hop_key(T.KEYS[1]))
    rule = [HC.retried_rule(bytes(frames[i]), int(lens[i]), SLOT, 128) for i in range(n)]
    sure, open_ = rule.count(True), rule.count(None)
    assert sure > 20 and len(np.unique(ov)) >= 5 and (out != frames).any(axis=1).sum() > 50
    try:
        with fresh_ctx() as ctx:
            router_setup(ctx, v6=True)
            judge = device_router(ctx, "ipv6", frames, lens, ifidx)
            orc.assert_br_equal(judge[:4], judge[4], (oa, ov, oe, os_), out, "hfv_br_process against the oracle")
            hfv.Ctx.debug_br_host_chunk(128)
            got = host_router(ctx, frames, lens, ifidx, 128, (oa, ov, oe, os_, out), "ipv6")
            assert got[0] == 3 and got[3] == 1 and sure <= got[2] <= sure + open_, got
            assert 128 < sure and sure + open_ <= 256 and got[1] == 2, got     # two rounds either way
    finally:
        reset_hooks()
