"""The model of tests/host_chunks.py held on the CPU, so that tests/test_gpu_host_chunks.py cannot
become vacuous: the restated schedule on cases worked out by hand, the asserted table against the
model, every retried count against the parser's rule (window 64) and against "hop field past byte
256" (window 256), the placement against the oracle router on the whole frames (and the reference
program where it is built), the conditions on the record corpora, and the test hooks' exports and
argument checks.

The schedule and the host worker pool themselves (csrc/hfv_host_pipe.h, free of HIP) run here too:
tests/host_pipe_driver.cpp, built under the thread sanitizer and under the address and undefined-
behaviour sanitizers, prints what two_slot_chunks calls, which must be what the model says."""
import ctypes
import errno
import os
import re
import subprocess

import pytest

import numpy as np

import br_topo as T
import frames_hostmem as H
import hf_bits as HB
import host_chunks as HC
import orc
import scion_hfv as hfv
from conftest import ROOT

HOOKS = ("hfv_debug_records_host_chunk", "hfv_debug_br_host_chunk", "hfv_debug_host_inline_rows",
         "hfv_debug_host_chunk_counts")
NAMES = tuple(HC.corpus_plans())


# ---- the schedule ------------------------------------------------------------------------------

def test_schedule_by_hand():
    assert HC.schedule(1, 128) == [(0, 0, 0, 1, 1)]
    assert HC.schedule(128, 128) == [(0, 0, 0, 128, 2)]
    assert HC.schedule(385, 128) == [(0, 0, 0, 128, 2), (1, 1, 128, 128, 2), (2, 0, 256, 128, 2), (3, 1, 384, 1, 1)]
    assert HC.schedule(229, 64) == [(0, 0, 0, 64, 1), (1, 1, 64, 64, 1), (2, 0, 128, 64, 1), (3, 1, 192, 37, 1)]
    assert HC.schedule(677, 100)[-1] == (6, 0, 600, 77, 2)
    assert HC.events(129, 128) == [("launch", 0), ("launch", 1), ("retire", 0), ("retire", 1)]
    assert HC.events(385, 128) == [("launch", 0), ("launch", 1), ("retire", 0), ("launch", 2), ("retire", 1),
                                   ("launch", 3), ("retire", 2), ("retire", 3)]
    for n, chunk, reuses in ((1, 128, 0), (256, 128, 0), (257, 128, 1), (385, 128, 2), (677, 128, 4), (677, 100, 5)):
        assert HC.slot_reuses(n, chunk) == reuses
        assert HC.retire_order(n, chunk) == list(range(-(-n // chunk)))


def test_retry_rounds_by_hand():
    mask = np.zeros(20, dtype=bool)
    assert HC.retry_rounds(mask, 4) == ([], 0)
    mask[[1, 2, 5, 7, 11, 13, 19]] = True
    rounds, cap = HC.retry_rounds(mask, 4)
    assert cap == 4 and [r.tolist() for r in rounds] == [[1, 2, 5, 7], [11, 13, 19]]
    rounds, cap = HC.retry_rounds(mask, 100)
    assert cap == 7 and [r.tolist() for r in rounds] == [[1, 2, 5, 7, 11, 13, 19]]
    mask[19] = False
    mask[3] = mask[4] = True                            # 8 = 2 * cap: two full rounds, nothing left over
    rounds, cap = HC.retry_rounds(mask, 4)
    assert cap == 4 and [len(r) for r in rounds] == [4, 4]
    assert HC.counts(20, 8, mask) == (3, 1, 8, 1) and HC.counts(20, 4, mask) == (5, 2, 8, 3)
    assert HC.counts(20, 8) == (3, 0, 0, 1)
    assert HC.retried_per_chunk(mask, 8) == (6, 2, 0)


# ---- the asserted table ------------------------------------------------------------------------

def test_table_matches_the_model():
    assert list(HC.TABLE) == HC.rows()
    for row in HC.rows():
        assert HC.model_row(*row) == HC.TABLE[row], row
    sizes = {(name, n, chunk) for name, n, chunk, _ in HC.TABLE}
    assert {("mix", n, 128) for n in (1, 127, 128, 129, 256, 257, 384, 385, 5 * 128 + 37)} <= sizes
    assert ("mix", 677, 100) in sizes
    for name, n, chunk in sizes:
        assert {w for a, b, c, w in HC.TABLE if (a, b, c) == (name, n, chunk)} >= {64, 256}
    assert {w for name, _, _, w in HC.TABLE if name == "mix"} == {64, 128, 136, 256, 0, HC.SLOT}


def parser_rule_64(frames, lens):
    """Window 64 by frames_hostmem.parse alone: no parse succeeds inside 64 bytes, so a frame is run
    again iff its clamped parse stops at a bound the whole frame reaches."""
    out = []
    for i in range(len(frames)):
        end = min(int(lens[i]), frames.shape[1])
        status, _, _, stop = H.parse(bytes(frames[i]), min(end, 64))
        assert stop[0] != "ok" and H.MIN_OK_END > 64
        out.append(stop[0] == "bound" and stop[1] <= end)
    return np.array(out)


def test_retried_counts_by_the_rules():
    for (name, n, chunk, window), (_, _, per_chunk, rounds) in HC.TABLE.items():
        frames, lens, _ = HC.corpus_prefix(name, n)
        if window == 64:
            mask = parser_rule_64(frames, lens)
            assert np.array_equal(mask, HC.corpus_plans()[name][0][:n]), (name, n)
        elif window in (256, 0):
            mask = HC.hop_field_past_256(frames, lens)
            assert sorted(np.nonzero(mask)[0]) == [i for i in HC.corpus_plans()[name][1] if i < n]
        elif window == HC.SLOT:
            mask = np.zeros(n, dtype=bool)
        else:
            continue
        assert HC.retried_per_chunk(mask, chunk) == per_chunk, (name, n, chunk, window)
        assert len(HC.retry_rounds(mask, chunk)[0]) == rounds, (name, n, chunk, window)


def test_placement_at_window_64():
    mix = HC.TABLE[("mix", HC.MIX_N, 128, 64)][2]
    assert 128 in mix and 0 in mix                                     # a chunk of retried frames only, one with none
    mask = HC.corpus_plans()["mix"][0]
    assert mask[0] and mask[127] and mask[384] and mask[511]           # first and last of a chunk
    assert not mask[125] and not mask[385]
    totals = {name: sum(HC.TABLE[(name, 385, 128, 64)][2]) for name in ("r127", "r128", "r129", "r256")}
    assert totals == {"r127": 127, "r128": 128, "r129": 129, "r256": 256}
    assert [HC.TABLE[(name, 385, 128, 64)][3] for name in ("r127", "r128", "r129", "r256")] == [1, 1, 2, 2]
    assert HC.retry_rounds(HC.corpus_plans()["r127"][0], 128)[1] == 127    # an odd cap
    assert np.nonzero(HC.corpus_plans()["r256"][0])[0][-1] < 384       # frames after the last full round
    assert HC.TABLE[("mix", HC.MIX_N, 100, 64)][3] == 4 and sum(HC.TABLE[("mix", HC.MIX_N, 100, 64)][2]) == 348


def test_no_frame_is_ambiguous():
    for name in NAMES:
        frames, lens, _ = HC.corpus(name)
        for window in HC.WINDOWS:
            HC.retried_mask(frames, lens, window)                      # asserts


# ---- the placement against the oracle router ---------------------------------------------------

def test_placement_against_the_oracle():
    """A frame the rule calls final at a window has, with its length cut to the window, the whole
    frame's action, verdict, egress and rewritten bytes: nothing past the window decides it.  The
    long-path frames are forwarded, the EtherType frames passed up as NOT_SCION, and every chunk of
    every row differs from every other in results and in rewritten bytes."""
    cfg, hk = T.br_config("br1"), orc.hop_key(T.KEYS[1])
    for name in NAMES:
        frames, lens, ifidx = HC.corpus(name)
        n = len(frames)
        a, v, e, _, out = HC.oracle(name, n)
        for window in HC.RULE_WINDOWS:
            final = ~HC.retried_mask(frames, lens, window)
            cut = frames.copy()
            ca, cv, ce, _ = orc.br_process(cut, np.minimum(lens, window), ifidx, cfg, hk)
            same = (ca == a) & (cv == v) & (ce == e) & (cut == out).all(axis=1)
            assert same[final].all(), (name, window, np.nonzero(final & ~same)[0][:8])
            assert (~same[~final]).any(), (name, window)
        longs = list(HC.corpus_plans()[name][1])
        assert (a[longs] == 4).all() and (v[longs] == hfv.VERDICT["SCION_FORWARD"]).all()
        eth = np.nonzero((frames[:, 12:14] == np.frombuffer(HC.ETHERTYPE_REJECTED, np.uint8)).all(axis=1))[0]
        assert len(eth) > 50 and (a[eth] == 2).all() and (v[eth] == hfv.VERDICT["NOT_SCION"]).all()
        assert len(np.unique(v)) >= 6 and (out != frames).any(axis=1).sum() > 50
    for name, n, chunk in sorted({row[:3] for row in HC.TABLE}):
        assert HC.chunks_distinct(name, n, chunk), (name, n, chunk)


def test_oracle_against_the_reference_program():
    if not orc.ref_br_available():
        return                                                         # no reference build in this checkout
    for name in NAMES:
        frames, lens, ifidx = HC.corpus(name)
        a, v, e, s, out = HC.oracle(name, len(frames))
        prog = frames.copy()
        res = orc.ref_br_process(prog, lens, ifidx, T.br_config("br1"), orc.hop_key(T.KEYS[1]))
        orc.assert_br_equal((a, v, e, s), out, res, prog, name)


# ---- the record corpora ------------------------------------------------------------------------

def test_record_corpora_hold_their_conditions():
    for keysel in (0, 1):
        for layout in HB.LAYOUTS:
            c = HB.corpus(keysel, layout)
            n = len(c.recs)
            step = HC.HF_STEP[(keysel, layout)]
            assert np.gcd(step, n) == 1 and HC.search_hf_step(keysel, layout) == step
            recs, passes, partial = HC.hf_dealt(keysel, layout)
            assert sorted(map(bytes, recs)) == sorted(map(bytes, c.recs)) and passes.sum() == c.passes.sum()
            for chunk in HC.REC_CHUNKS:
                assert HC.mixed_and_distinct(passes, chunk), (keysel, layout, chunk)
                assert not keysel or HC.mixed_and_distinct(partial, chunk)
                assert 3 * chunk + 37 < n
            assert passes[list(HC.ONE_RECORD_CHUNKS)].all()
    assert not HC.mixed_and_distinct(HB.corpus(0).passes, 64)          # why the corpus is dealt, not rolled
    assert HC.kt_roll_ok(HC.KT_ROLL)
    recs, want = HC.kt_rolled()
    assert len(recs) == len(want["A"]) == 4500


def test_mixed_and_distinct_sees_what_it_must():
    p = np.array(([True, False] * 32 + [False, True] * 32) * 2)
    assert HC.mixed_and_distinct(p[:128], 64) and not HC.mixed_and_distinct(p, 64)      # chunks 0 and 2 are equal
    assert not HC.mixed_and_distinct(np.concatenate([p[:64], np.ones(64, dtype=bool)]), 64)
    assert not HC.mixed_and_distinct(np.concatenate([p[:64], np.zeros(3, dtype=bool)]), 64)


# ---- the hooks ---------------------------------------------------------------------------------

def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_hooks_only_in_the_test_build():
    assert set(HOOKS) <= _exports(hfv.TEST_LIB_PATH)
    assert not set(HOOKS) & _exports(hfv.LIB_PATH)


def test_hook_arguments():
    L = ctypes.CDLL(hfv.TEST_LIB_PATH)
    sz, E = ctypes.c_size_t, -errno.EINVAL
    try:
        assert L.hfv_debug_records_host_chunk(sz(100)) == E            # not a multiple of 64
        assert L.hfv_debug_records_host_chunk(sz((1 << 18) + 64)) == E
        assert L.hfv_debug_br_host_chunk(sz((1 << 16) + 1)) == E
        for ok in (64, 128, 1 << 18, 0):
            assert L.hfv_debug_records_host_chunk(sz(ok)) == 0
        for ok in (1, 100, 128, 1 << 16, 0):
            assert L.hfv_debug_br_host_chunk(sz(ok)) == 0
        for ok in (16, 1, 0):
            assert L.hfv_debug_host_inline_rows(sz(ok)) == 0
        out = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        assert L.hfv_debug_host_chunk_counts(out) == 0 and list(out) == [0, 0, 0, 0]    # no host call yet
        assert L.hfv_debug_host_chunk_counts(None) == E
    finally:
        L.hfv_debug_records_host_chunk(sz(0))
        L.hfv_debug_br_host_chunk(sz(0))
        L.hfv_debug_host_inline_rows(sz(0))


# ---- the real schedule and the real pool, as a host program under the sanitizers ---------------

BY_HAND = ((1, 128), (128, 128), (385, 128), (229, 64), (677, 100), (129, 128), (256, 128), (257, 128), (677, 128))
PAIRS = BY_HAND + tuple((n, chunk) for n in (1, 63, 64, 65, 128, 129, 385, 677) for chunk in (64, 100, 128))


@pytest.fixture(scope="module", params=["thread", "address,undefined"])
def pipe_driver(request, tmp_path_factory):
    """tests/host_pipe_driver.cpp over csrc/hfv_host_pipe.h, built with -fsanitize=<param>; run(*args)
    runs it (nothing preloaded) and returns its output lines.  A sanitizer report fails the run."""
    exe = str(tmp_path_factory.mktemp("host_pipe") / "host_pipe_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=" + request.param, "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "scion-xdp-br_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "host_pipe_driver.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and re.search(r"sanitize|[atu]b?san", b.stderr):
        pytest.skip("sanitizer runtime unavailable: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66", ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr, (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()
    return run


def _cases(lines):
    """{(n, chunk): ([(call, slot, first, count) | ("wait", slot)], rc, reuses)} of the driver's output."""
    out, key = {}, None
    for line in lines:
        w = line.split()
        if w[0] == "case":
            key = (int(w[1]), int(w[2]))
            out[key] = [[], None, None]
        elif w[0] == "end":
            out[key][1:] = int(w[1]), int(w[2])
        else:
            out[key][0].append((w[0],) + tuple(int(x) for x in w[1:]))
    return out


def _model_calls(n, chunk, upto=None):
    """What two_slot_chunks must call, by HC.events and HC.schedule (upto: stop after that launch)."""
    sched = HC.schedule(n, chunk)
    out = []
    for kind, c in HC.events(n, chunk):
        _, slot, first, cnt, _ = sched[c]
        if kind == "retire":
            out.append(("wait", slot))
        out.append((kind, slot, first, cnt))
        if kind == "launch" and c == upto:
            break
    return out


def test_driver_runs_the_model_schedule(pipe_driver):
    assert len(set(PAIRS)) == 8 * 3 + 3                                # the grid and by-hand's three outside it
    got = _cases(pipe_driver("sched", *[x for pair in dict.fromkeys(PAIRS) for x in pair]))
    assert set(got) == set(PAIRS)
    for (n, chunk), (calls, rc, reuses) in got.items():
        assert calls == _model_calls(n, chunk), (n, chunk)
        assert rc == 0 and reuses == HC.slot_reuses(n, chunk) == HC.counts(n, chunk)[3], (n, chunk)
        assert [c[2] // chunk for c in calls if c[0] == "retire"] == HC.retire_order(n, chunk)
        assert [c[1:] for c in calls if c[0] == "launch"] == [s[1:4] for s in HC.schedule(n, chunk)]


def test_driver_stops_at_the_first_error(pipe_driver):
    """submit fails on chunk 2 of 7: the driver returns its code and calls nothing more: chunks 1 and 2
    are neither waited for nor retired."""
    (key, (calls, rc, reuses)), = _cases(pipe_driver("fail", 677, 100, 2, -5)).items()
    assert key == (677, 100) and rc == -5 and reuses == 1
    assert calls == _model_calls(677, 100, upto=2) and calls[-1] == ("launch", 0, 200, 100)
    assert [c for c in calls if c[0] == "retire"] == [("retire", 0, 0, 100)]
    # a failure in the last chunk leaves the two chunks in flight unretired as well
    (_, (calls, rc, _)), = _cases(pipe_driver("fail", 385, 128, 3, 7)).items()
    assert rc == 7 and calls == _model_calls(385, 128, upto=3)


def test_pool_touches_every_row_once(pipe_driver):
    """1, 3 and 8 threads, 0, 1, 7, 8 and 4097 rows, through parallel_rows (inline and through the pool)
    and HostPool::run: every row once, by counters that are not atomic."""
    assert pipe_driver("pool") == ["pool ok"]


def test_pool_back_to_back_jobs(pipe_driver):
    """2000 jobs on one pool of 8: the generation and countdown hand-off, under the thread sanitizer
    with no report (and under the address sanitizer)."""
    assert pipe_driver("stress", 2000) == ["stress ok 2000"]
