"""Shared by test_host_chunks.py and test_gpu_host_chunks.py: the chunk pipelines of the two chunked
host paths (hfv_verify_records_host, hfv_br_process_host) restated in plain Python, the corpora both
modules run, and the asserted table of what every router row must run.  Test infrastructure only;
independent of the C and HIP code.

The schedule.  Both paths cut n items into chunks of `chunk` (the last one ragged) and run them on two
alternating stream slots: the loop visits c = 0 .. nchunks + 1; at c >= 2 it first retires chunk c - 2
(same slot: waits for the slot's stream and copies the chunk's results to where the chunk began), then,
while c < nchunks, launches chunk c on slot c & 1.  A chunk with c >= 2 reuses a slot within the call.
The router then packs the frames marked HFV_BR_ACTION_RETRY, in order, into rounds of at most
cap = min(retried, chunk) frames, runs every round whole (stream slot 0) and scatters its results back.

The router's retry rule (retried_rule): the windowed pass gives the kernel min(len, slot, window) bytes
of each frame; a bounds check ("data + x > data_end", br/src/bpf/parser.h) that fails at an x the whole
frame still holds (x <= min(len, slot)) marks the frame for the second pass.  The parser's checks are
those of frames_hostmem.parse.  After a parse that succeeds the router has two more: the next hop
field at a segment switch (hf + 24) and the second info field (inf + 16); whether a frame reaches them
depends on the router tables, so a frame whose window ends between its parse and those is ambiguous
and the corpora here hold none (decided at 128, 136 and 256; no parse succeeds inside 64 bytes, so
there the parser's rule alone decides).

Record corpora.  hf_bits.corpus(keysel, layout) begins with 2048 passing records in a row, so no roll
of it has mixed verdicts in every chunk of 64; it is dealt instead: record i of the dealt corpus is
record i * step mod n, with the step (HF_STEP, coprime to n) chosen so that at chunk 64 and 128 no
chunk's verdicts are all 0 or all ones, no two chunks have equal verdict words, and records 64, 128
and 256 (the one-record ragged chunks) pass.  The three-table corpus of key_tables.py is rolled by
KT_ROLL: the same, under each table, and in every chunk the three tables' verdict words differ.

Router corpus.  Slot 1024, IPv4 fuzz frames (br_fuzz.fuzz_batch, payload_max=600), the long-path frames
of br_fuzz (hop field past byte 256: retried at every window below the slot) and frames the parser
rejects by EtherType (decided inside any window).  A boolean mask says which positions hold a frame
retried at window 64; corpus_plans lists the masks (see there)."""
import functools
import math

import numpy as np

import br_fuzz as F
import br_topo as T
import frames_hostmem as H
import frames_rx_ref as R
import hf_bits as HB
import key_tables as KT
import orc

REC_CHUNK_DEFAULT = 1 << 18
BR_CHUNK_DEFAULT = 1 << 16
REC_CHUNKS = (64, 128)


# ---- the schedule ------------------------------------------------------------------------------

def schedule(n, chunk):
    """[(chunk index, stream slot, first, count, bitmap words)]"""
    out = []
    for c in range((n + chunk - 1) // chunk):
        first = c * chunk
        cnt = min(chunk, n - first)
        out.append((c, c & 1, first, cnt, (cnt + 63) // 64))
    return out


def events(n, chunk):
    """The loop in order: [("retire" | "launch", chunk index)]."""
    nchunks = (n + chunk - 1) // chunk
    out = []
    for c in range(nchunks + 2):
        if c >= 2:
            out.append(("retire", c - 2))
        if c < nchunks:
            out.append(("launch", c))
    return out


def retire_order(n, chunk):
    return [c for kind, c in events(n, chunk) if kind == "retire"]


def slot_reuses(n, chunk):
    return sum(1 for kind, c in events(n, chunk) if kind == "launch" and c >= 2)


def retry_rounds(mask, chunk):
    """([frame indices of each round], cap) of the router's second pass."""
    idx = np.nonzero(np.asarray(mask, dtype=bool))[0]
    if not len(idx):
        return [], 0
    cap = min(len(idx), chunk)
    return [idx[k:k + cap] for k in range(0, len(idx), cap)], cap


def counts(n, chunk, mask=None):
    """What hfv_debug_host_chunk_counts must report: (chunks, retry rounds, retried, slot reuses)."""
    rounds = retry_rounds(mask, chunk)[0] if mask is not None else []
    return (len(schedule(n, chunk)), len(rounds), int(np.sum(mask)) if mask is not None else 0, slot_reuses(n, chunk))


def retried_per_chunk(mask, chunk):
    return tuple(int(np.sum(mask[first:first + cnt])) for _, _, first, cnt, _ in schedule(len(mask), chunk))


# ---- record corpora ----------------------------------------------------------------------------

def rec_sizes(full, chunk):
    return (full, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 37)


def chunk_words(passes, chunk):
    """The verdict words of every chunk of passes: [bytes]."""
    return [HB.bitmap(passes[first:first + cnt]).tobytes() for _, _, first, cnt, _ in schedule(len(passes), chunk)]


def mixed_and_distinct(passes, chunk):
    """No chunk's verdicts all 0 or all ones, no two chunks with equal verdict words."""
    parts = [passes[first:first + cnt] for _, _, first, cnt, _ in schedule(len(passes), chunk)]
    words = chunk_words(passes, chunk)
    return all(p.any() and not p.all() for p in parts) and len(set(words)) == len(words)


# (keysel, layout) -> step of the deal; found by search_hf_step, held by test_host_chunks.py
HF_STEP = {
    (0, (40, 48, 64)): 65, (0, (0, 8, 24)): 33, (0, (8, 16, 72)): 75,
    (1, (40, 48, 64)): 65, (1, (0, 8, 24)): 33, (1, (8, 16, 72)): 75,
}
ONE_RECORD_CHUNKS = (64, 128, 256)     # n = chunk + 1 and 2 * chunk + 1: the ragged chunk's only record


def hf_deal_ok(c, order):
    passes = c.passes[order]
    ok = all(mixed_and_distinct(passes, chunk) for chunk in REC_CHUNKS) and passes[list(ONE_RECORD_CHUNKS)].all()
    if ok and c.keysel:
        ok = all(mixed_and_distinct(HB.partial_passes(c)[order], chunk) for chunk in REC_CHUNKS)
    return ok


def search_hf_step(keysel, layout):
    c = HB.corpus(keysel, tuple(layout))
    n = len(c.recs)
    for step in range(3, n, 2):
        if math.gcd(step, n) == 1 and hf_deal_ok(c, (np.arange(n) * step) % n):
            return step
    raise AssertionError("no step")


@functools.lru_cache(maxsize=None)
def hf_dealt(keysel, layout):
    """(records u8[n, stride], passes bool[n], partial passes bool[n]) of the dealt hf_bits corpus."""
    layout = tuple(layout)
    c = HB.corpus(keysel, layout)
    n = len(c.recs)
    order = (np.arange(n) * HF_STEP[(keysel, layout)]) % n
    out = (np.ascontiguousarray(c.recs[order]), c.passes[order].copy(), HB.partial_passes(c)[order].copy())
    for a in out:
        a.setflags(write=False)
    return out


KT_ROLL = 0


def kt_roll_ok(roll):
    want = {name: np.roll(KT.want_bool()[name], roll) for name in KT.NAMES}
    for chunk in REC_CHUNKS:
        if not all(mixed_and_distinct(want[name], chunk) for name in KT.NAMES):
            return False
        w = [chunk_words(want[name], chunk) for name in KT.NAMES]
        if any(len({w[0][k], w[1][k], w[2][k]}) != 3 for k in range(len(w[0]))):
            return False
    return True


@functools.lru_cache(maxsize=None)
def kt_rolled():
    """(records u8[N, 64], {table name: passes bool[N]}) of the rolled three-table corpus."""
    recs = np.ascontiguousarray(np.roll(KT.corpus()[0], KT_ROLL, axis=0))
    recs.setflags(write=False)
    want = {}
    for name in KT.NAMES:
        want[name] = np.roll(KT.want_bool()[name], KT_ROLL)
        want[name].setflags(write=False)
    return recs, want


# ---- the router's retry rule -------------------------------------------------------------------

SLOT = 1024
WINDOWS = (64, 128, 136, 256, 0, SLOT)          # 0: the default, min(256, slot)
RULE_WINDOWS = (64, 128, 136, 256)


def eff_window(window, slot=SLOT):
    return min(256, slot) if window == 0 else window


def retried_rule(row: bytes, ln: int, slot: int, window: int):
    """True / False: the windowed pass marks the frame for the second pass or not; None: that depends
    on the router tables (see the module text)."""
    end = min(ln, slot)
    lim = min(end, window)
    _, inf, hf, stop = H.parse(row, lim)
    if stop[0] == "bound":
        return stop[1] <= end
    if stop[0] == "value":
        return False
    if any(lim < x <= end for x in (hf + 24, inf + 16)):
        return None
    return False


def retried_mask(frames, lens, window):
    """bool[n] by retried_rule; no frame may be ambiguous."""
    slot = frames.shape[1]
    out = [retried_rule(bytes(frames[i]), int(lens[i]), slot, eff_window(window, slot)) for i in range(len(frames))]
    assert None not in out, "ambiguous frame %d at window %d" % (out.index(None), window)
    return np.array(out, dtype=bool)


def hop_field_past_256(frames, lens):
    """bool[n]: the whole frame parses and its current hop field ends past byte 256 (the long-path
    frames): the frames retried at window 256."""
    out = []
    for i in range(len(frames)):
        st, _, hf, _ = H.parse(bytes(frames[i]), min(int(lens[i]), frames.shape[1]))
        out.append(st == H.OK and hf + 12 > 256)
    return np.array(out, dtype=bool)


# ---- the router corpus -------------------------------------------------------------------------

POOL_N = 3000
POOL_SEED = 41
ETHERTYPE_REJECTED = b"\x88\xb5"     # IEEE local experimental: neither IPv4 nor IPv6


@functools.lru_cache(maxsize=None)
def pools():
    """(retried, final, longs): lists of (frame bytes, length, ifindex).  retried / final: fuzz frames
    by the rule at window 64, without those ambiguous at a larger window and those retried at 256
    (only the long-path frames are); longs: br_fuzz.long_path_frames."""
    frames, lens, ifidx = F.fuzz_batch(R.hop_inputs(False), "br1", False, POOL_N, POOL_SEED, slot=SLOT, payload_max=600)
    retried, final = [], []
    for i in range(POOL_N):
        row, ln = bytes(frames[i]), int(lens[i])
        rule = [retried_rule(row, ln, SLOT, w) for w in RULE_WINDOWS]
        if None in rule or rule[3]:
            continue
        (retried if rule[0] else final).append((row[:max(ln, 14)], ln, int(ifidx[i])))
    longs = [(f, len(f), i) for f, i in F.long_path_frames(False, R.MAC)]
    return retried, final, longs


C = 128
MIX_N = 5 * C + 37
SIZES = (1, 127, 128, 129, 256, 257, 384, 385, MIX_N)     # at chunk 128; MIX_N also at chunk 100


def _mix_mask():
    """Chunk 0: every third frame and the last (a retried frame first and last in a chunk); chunk 1:
    only retried frames; chunk 2: none; chunk 3: every second and the last; chunk 4: four of five;
    the ragged chunk 5: one of four."""
    i = np.arange(MIX_N)
    j = i % C
    m = np.zeros(MIX_N, dtype=bool)
    m |= (i < C) & ((j % 3 == 0) | (j == C - 1))
    m |= (i >= C) & (i < 2 * C)
    m |= (i >= 3 * C) & (i < 4 * C) & ((j % 2 == 0) | (j == C - 1))
    m |= (i >= 4 * C) & (i < 5 * C) & (j % 5 != 0)
    m |= (i >= 5 * C) & (j % 4 == 1)
    return m


def _spread_mask(n, per_chunk, seed):
    """per_chunk[c] retried frames at seeded positions of chunk c (chunks of C)."""
    m = np.zeros(n, dtype=bool)
    rng = np.random.default_rng(seed)
    for (_, _, first, cnt, _), k in zip(schedule(n, C), per_chunk):
        m[first + np.sort(rng.permutation(cnt)[:k])] = True
    return m


# name -> (mask at window 64, positions of the long-path frames, first pool entry used)
# r127 / r128 / r129 / r256: cap - 1 (an odd cap: the bounce buffer's parts at odd counts), cap, cap + 1
# and exactly 2 * cap retried frames in 3 * 128 + 1 frames; r256 ends with frames that are not retried,
# so the round loop meets an empty round after its two full ones.
@functools.lru_cache(maxsize=None)
def corpus_plans():
    plans = {"mix": (_mix_mask(), (0, 127, 128, 255, 384, 511, 513, 641), 0)}
    for k, (name, per_chunk) in enumerate((("r127", (60, 40, 26, 1)), ("r128", (64, 33, 30, 1)),
                                           ("r129", (50, 48, 30, 1)), ("r256", (128, 100, 28, 0)))):
        m = _spread_mask(3 * C + 1, per_chunk, 7 + k)
        at = np.nonzero(m)[0]
        plans[name] = (m, (int(at[0]), int(at[len(at) // 2])), 400 * (k + 1))
    return plans


@functools.lru_cache(maxsize=None)
def corpus(name):
    """(frames u8[n, SLOT], lens u16[n], ifindex u32[n]) of a plan, read-only: the long-path frames at
    their positions, the next retried pool frame at every other position of the mask, and at the
    rest by turns a final pool frame and a retried one with its EtherType replaced."""
    mask, longs_at, start = corpus_plans()[name]
    retried, final, longs = pools()
    n = len(mask)
    frames = np.zeros((n, SLOT), np.uint8)
    lens = np.zeros(n, np.uint16)
    ifidx = np.zeros(n, np.uint32)
    r = f = start
    nf = 0
    for i in range(n):
        if i in longs_at:
            row, ln, ifi = longs[longs_at.index(i) % len(longs)]
        elif mask[i]:
            row, ln, ifi = retried[r % len(retried)]
            r += 1
        elif nf % 2 == 0:
            row, ln, ifi = final[f % len(final)]
            f += 1
            nf += 1
        else:
            row, ln, ifi = retried[(r + 1000 + nf) % len(retried)]
            row = row[:12] + ETHERTYPE_REJECTED + row[14:]
            nf += 1
        frames[i, :len(row)] = np.frombuffer(row, np.uint8)
        lens[i], ifidx[i] = ln, ifi
    for a in (frames, lens, ifidx):
        a.setflags(write=False)
    return frames, lens, ifidx


def corpus_prefix(name, n):
    frames, lens, ifidx = corpus(name)
    return frames[:n], lens[:n], ifidx[:n]


@functools.lru_cache(maxsize=None)
def oracle(name, n):
    """(action, verdict, egress, stats, rewritten frames) of orc.br_process on the whole frames."""
    frames, lens, ifidx = corpus_prefix(name, n)
    out = frames.copy()
    a, v, e, s = orc.br_process(out, lens, ifidx, T.br_config("br1"), orc.hop_key(T.KEYS[1]))
    for x in (a, v, e, s, out):
        x.setflags(write=False)
    return a, v, e, s, out


def chunks_distinct(name, n, chunk):
    """No two chunks with equal (action, verdict, egress) vectors, none with equal rewritten bytes
    (where and to what)."""
    frames, _, _ = corpus_prefix(name, n)
    a, v, e, _, out = oracle(name, n)
    res, rew = [], []
    for _, _, first, cnt, _ in schedule(n, chunk):
        s = slice(first, first + cnt)
        res.append(a[s].tobytes() + v[s].tobytes() + e[s].tobytes())
        changed = out[s] != frames[s]
        rew.append(changed.tobytes() + out[s][changed].tobytes())
    return len(set(res)) == len(res) and len(set(rew)) == len(rew)


def rows():
    """Every (corpus, n, chunk, window) the GPU module runs."""
    out = [("mix", n, C, w) for n in SIZES for w in WINDOWS]
    out += [("mix", MIX_N, 100, w) for w in WINDOWS]
    out += [(name, 3 * C + 1, C, w) for name in ("r127", "r128", "r129", "r256") for w in (64, 256)]
    return out


def model_row(name, n, chunk, window):
    """(chunks, slot reuses, retried frames per chunk, retry rounds) by the schedule and the rule."""
    frames, lens, _ = corpus_prefix(name, n)
    mask = retried_mask(frames, lens, window)
    return len(schedule(n, chunk)), slot_reuses(n, chunk), retried_per_chunk(mask, chunk), len(retry_rounds(mask, chunk)[0])


# (corpus, n, chunk, window): (chunks, slot reuses, retried frames per chunk, retry rounds)
TABLE = {
    ('mix', 1, 128, 64): (1, 0, (1,), 1),
    ('mix', 1, 128, 128): (1, 0, (1,), 1),
    ('mix', 1, 128, 136): (1, 0, (1,), 1),
    ('mix', 1, 128, 256): (1, 0, (1,), 1),
    ('mix', 1, 128, 0): (1, 0, (1,), 1),
    ('mix', 1, 128, 1024): (1, 0, (0,), 0),
    ('mix', 127, 128, 64): (1, 0, (43,), 1),
    ('mix', 127, 128, 128): (1, 0, (3,), 1),
    ('mix', 127, 128, 136): (1, 0, (3,), 1),
    ('mix', 127, 128, 256): (1, 0, (1,), 1),
    ('mix', 127, 128, 0): (1, 0, (1,), 1),
    ('mix', 127, 128, 1024): (1, 0, (0,), 0),
    ('mix', 128, 128, 64): (1, 0, (44,), 1),
    ('mix', 128, 128, 128): (1, 0, (4,), 1),
    ('mix', 128, 128, 136): (1, 0, (4,), 1),
    ('mix', 128, 128, 256): (1, 0, (2,), 1),
    ('mix', 128, 128, 0): (1, 0, (2,), 1),
    ('mix', 128, 128, 1024): (1, 0, (0,), 0),
    ('mix', 129, 128, 64): (2, 0, (44, 1), 1),
    ('mix', 129, 128, 128): (2, 0, (4, 1), 1),
    ('mix', 129, 128, 136): (2, 0, (4, 1), 1),
    ('mix', 129, 128, 256): (2, 0, (2, 1), 1),
    ('mix', 129, 128, 0): (2, 0, (2, 1), 1),
    ('mix', 129, 128, 1024): (2, 0, (0, 0), 0),
    ('mix', 256, 128, 64): (2, 0, (44, 128), 2),
    ('mix', 256, 128, 128): (2, 0, (4, 7), 1),
    ('mix', 256, 128, 136): (2, 0, (4, 6), 1),
    ('mix', 256, 128, 256): (2, 0, (2, 2), 1),
    ('mix', 256, 128, 0): (2, 0, (2, 2), 1),
    ('mix', 256, 128, 1024): (2, 0, (0, 0), 0),
    ('mix', 257, 128, 64): (3, 1, (44, 128, 0), 2),
    ('mix', 257, 128, 128): (3, 1, (4, 7, 0), 1),
    ('mix', 257, 128, 136): (3, 1, (4, 6, 0), 1),
    ('mix', 257, 128, 256): (3, 1, (2, 2, 0), 1),
    ('mix', 257, 128, 0): (3, 1, (2, 2, 0), 1),
    ('mix', 257, 128, 1024): (3, 1, (0, 0, 0), 0),
    ('mix', 384, 128, 64): (3, 1, (44, 128, 0), 2),
    ('mix', 384, 128, 128): (3, 1, (4, 7, 0), 1),
    ('mix', 384, 128, 136): (3, 1, (4, 6, 0), 1),
    ('mix', 384, 128, 256): (3, 1, (2, 2, 0), 1),
    ('mix', 384, 128, 0): (3, 1, (2, 2, 0), 1),
    ('mix', 384, 128, 1024): (3, 1, (0, 0, 0), 0),
    ('mix', 385, 128, 64): (4, 2, (44, 128, 0, 1), 2),
    ('mix', 385, 128, 128): (4, 2, (4, 7, 0, 1), 1),
    ('mix', 385, 128, 136): (4, 2, (4, 6, 0, 1), 1),
    ('mix', 385, 128, 256): (4, 2, (2, 2, 0, 1), 1),
    ('mix', 385, 128, 0): (4, 2, (2, 2, 0, 1), 1),
    ('mix', 385, 128, 1024): (4, 2, (0, 0, 0, 0), 0),
    ('mix', 677, 128, 64): (6, 4, (44, 128, 0, 65, 102, 9), 3),
    ('mix', 677, 128, 128): (6, 4, (4, 7, 0, 3, 6, 1), 1),
    ('mix', 677, 128, 136): (6, 4, (4, 6, 0, 3, 6, 1), 1),
    ('mix', 677, 128, 256): (6, 4, (2, 2, 0, 2, 1, 1), 1),
    ('mix', 677, 128, 0): (6, 4, (2, 2, 0, 2, 1, 1), 1),
    ('mix', 677, 128, 1024): (6, 4, (0, 0, 0, 0, 0, 0), 0),
    ('mix', 677, 100, 64): (7, 5, (34, 82, 56, 8, 50, 77, 41), 4),
    ('mix', 677, 100, 128): (7, 5, (2, 8, 1, 1, 1, 7, 1), 1),
    ('mix', 677, 100, 136): (7, 5, (2, 7, 1, 1, 1, 7, 1), 1),
    ('mix', 677, 100, 256): (7, 5, (1, 2, 1, 1, 0, 2, 1), 1),
    ('mix', 677, 100, 0): (7, 5, (1, 2, 1, 1, 0, 2, 1), 1),
    ('mix', 677, 100, 1024): (7, 5, (0, 0, 0, 0, 0, 0, 0), 0),
    ('r127', 385, 128, 64): (4, 2, (60, 40, 26, 1), 1),
    ('r127', 385, 128, 256): (4, 2, (1, 1, 0, 0), 1),
    ('r128', 385, 128, 64): (4, 2, (64, 33, 30, 1), 1),
    ('r128', 385, 128, 256): (4, 2, (1, 1, 0, 0), 1),
    ('r129', 385, 128, 64): (4, 2, (50, 48, 30, 1), 2),
    ('r129', 385, 128, 256): (4, 2, (1, 1, 0, 0), 1),
    ('r256', 385, 128, 64): (4, 2, (128, 100, 28, 0), 2),
    ('r256', 385, 128, 256): (4, 2, (1, 1, 0, 0), 1),
}
