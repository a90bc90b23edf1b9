"""The tile dealing of k_verify_frames_list (csrc/hfv_frames_fused_kernel.hip) and the launch split
of hfv_verify_frames_batches (csrc/hfv_api.cpp) restated in plain Python, and the frame-batch lists
the tests run.  Shared by test_frames_list.py (CPU) and test_gpu_frames_list.py.

TEST INFRASTRUCTURE ONLY.

The model.  hfv_verify_frames_batches drops empty batches and cuts the rest, in list order, into
launches: a launch ends at BATCH_MAX batches, at 2^31 tiles and where the next batch is staged and
the launch is not, or the other way round (staged: slot >= 128, slot % 16 == 0, frames 16-byte
aligned).  A launch numbers its batches' 64-frame tiles one after the other (batch j holds global
tiles [cum[j], cum[j+1]), T = cum[nb]) and runs G = min(cap or CUs, ceil(T / W)) blocks of W waves
(16 under KEYSEL_ZERO, 12 under KEYSEL_IFID); block k owns tiles [T*k/G, T*(k+1)/G), its LDS counter
starts at 0 and every claim takes the next tile of the range (fused_deal.claims).  Which wave makes
which claim is decided at run time; where a wave's own sequence of tiles matters (the forward step
from one batch to a later one) the model takes the round-robin schedule, wave w making the claims
w, w + W, ...: one schedule the hardware may choose.

The lists.  Every batch is a slice of one of the six 4096-frame fuzz batches (frames_rx_ref.batch)
or of the window-edge corpus (br_shift.shift_corpus), put into slots of the batch's own size.  The
judge is hfv_frame_extract per frame and the record checker (frames_rx_ref.frame_extract,
oracle_bits), per batch.  A slice's offset is moved forward to the first one at which the batch's
last frame passes: a lane past n that voted with the clamped last frame would set a bit at or past
n.  Everything is built once per process and left unchanged."""
import collections
import functools

import numpy as np

import br_shift as S
import br_topo as T
import frames_rx_ref as R
import fused_deal as FD
import orc

BATCH_MAX = 32                    # kFrameBatchMax: non-empty batches per launch
MAX_TILES = 1 << 31               # tiles per launch
WIN = 128                         # kFrWin: the staged bytes per frame
ISET = (5, 7)                     # the internal-ifindex set of every test
K1 = T.KEYS[1]
GRIDS = (1, 2, 3, FD.REAL_GRID)
KEYSELS = (0, 1)

# One batch of a list.  src: ("fuzz", br, v6) or ("corpus", br, v6); off, n: the slice; slot: the
# batch's slot size; ifx: 0 no ifindex array (NULL), 1 the source's own, 2 the source's rolled by one
# frame; status: with a status buffer; shift: bytes the frame buffer lies past a 16-byte boundary.
Spec = collections.namedtuple("Spec", "src off n slot ifx status shift", defaults=(2048, 1, True, 0))
EMPTY = Spec(None, 0, 0)

Deal = collections.namedtuple("Deal", "index n cum T G ranges staged")
Place = collections.namedtuple("Place", "launches mid_batch_start longest_step")


# ---- the model ----------------------------------------------------------------------------------

def stageable(slot, shift=0):
    return slot >= WIN and slot % 16 == 0 and shift % 16 == 0


def launches(specs):
    """[[(position in the list, n), ...], ...] and the launches' staged flags."""
    out, flags, cur, tiles, staged = [], [], [], 0, None
    for i, s in enumerate(specs):
        if s.n == 0:
            continue
        st, t = stageable(s.slot, s.shift), FD.tiles_of(s.n)
        if cur and (len(cur) == BATCH_MAX or tiles + t > MAX_TILES or st != staged):
            out.append(cur), flags.append(staged)
            cur, tiles = [], 0
        staged = st
        cur.append((i, s.n))
        tiles += t
    if cur:
        out.append(cur), flags.append(staged)
    return out, flags


def deal(launch, staged, keysel, cap=0, cus=FD.REAL_GRID):
    """One launch on at most `cap` (or `cus`) blocks: cum[], T, G and every block's tile range."""
    n = [m for _, m in launch]
    cum = [0]
    for m in n:
        cum.append(cum[-1] + FD.tiles_of(m))
    total, w = cum[-1], FD.WAVES[keysel]
    g = min(cap or cus, (total + w - 1) // w)
    return Deal([i for i, _ in launch], n, cum, total, g, [FD.block_range(total, g, k) for k in range(g)], staged)


def tile_of(d, g):
    """Global tile g of a launch -> (batch j of the launch, tile within it, frames in the tile)."""
    j = max(k for k in range(len(d.n)) if d.cum[k] <= g)
    t = g - d.cum[j]
    return j, t, min(64, d.n[j] - 64 * t)


def owners(d, keysel):
    """How often each (batch, tile) of the launch is verified, over all blocks' claims."""
    seen = collections.Counter()
    for k in range(d.G):
        taken, total = FD.claims(d.T, d.G, k, FD.WAVES[keysel])
        assert total == len(taken) + FD.WAVES[keysel]
        assert taken == list(range(*d.ranges[k]))
        for g in taken:
            seen[tile_of(d, g)[:2]] += 1
    return seen


def placement(specs, keysel, cap=0):
    """Where the list's batches fall against the block ranges: the number of launches, whether some
    block range starts in the middle of a batch, and the most batches one forward step of a wave
    passes under the round-robin schedule (1: into the next batch; 0: no wave changes batch)."""
    ls, flags = launches(specs)
    mid, longest = False, 0
    w = FD.WAVES[keysel]
    for launch, st in zip(ls, flags):
        d = deal(launch, st, keysel, cap)
        for lo, hi in d.ranges:
            mid |= lo not in d.cum
            for g in range(lo, hi - w):
                longest = max(longest, tile_of(d, g + w)[0] - tile_of(d, g)[0])
    return Place(len(ls), mid, longest)


# ---- sources and the judge ----------------------------------------------------------------------

def reslot(frames, slot):
    """The same frames in slots of `slot` bytes (longer frames are cut: len is clamped to slot)."""
    out = np.zeros((len(frames), slot), dtype=np.uint8)
    w = min(slot, frames.shape[1])
    out[:, :w] = frames[:, :w]
    return out


@functools.lru_cache(maxsize=None)
def source(src):
    """(frames, lens, ifindex) of a source, read-only."""
    kind, br, v6 = src
    if kind == "fuzz":
        b = R.batch(br, v6)
        return b.frames, b.lens, b.ifidx
    frames, lens, ifidx, _, _ = S.shift_corpus(v6)[br]
    return frames, lens, ifidx


@functools.lru_cache(maxsize=None)
def ifid_raw():
    """256 generated keys, the topology's AS interfaces 1..6 under the AS key."""
    raw = bytearray(orc.gen_key_table(256))
    for ifid in range(1, 7):
        raw[16 * ifid:16 * ifid + 16] = K1
    return bytes(raw)


@functools.lru_cache(maxsize=None)
def keys(keysel):
    """(raw keys, hop keys, valid words) the ctx holds under `keysel`."""
    raw = ifid_raw() if keysel else K1
    return (raw,) + orc.key_table(raw)


def judge(frames, lens, internal, keysel, valid=None, raw=None):
    """(bitmap words, status) of the frames by hfv_frame_extract per frame and the record checker,
    under the keys of keys(keysel) or of the raw key table `raw`."""
    hk, v = keys(keysel)[1:] if raw is None else orc.key_table(raw)
    st, inf, hf = R.frame_extract(np.ascontiguousarray(frames), lens, internal)
    return R.oracle_bits(st, inf, hf, hk, v if valid is None else valid, keysel), st


def ifindex_of(spec):
    """The batch's ifindex array (None: NULL)."""
    if not spec.ifx:
        return None
    ifidx = source(spec.src)[2]
    ifidx = np.roll(ifidx, 1) if spec.ifx == 2 else ifidx
    return np.ascontiguousarray(ifidx[spec.off:spec.off + spec.n])


Batch = collections.namedtuple("Batch", "spec frames lens ifidx")


@functools.lru_cache(maxsize=None)
def batch(spec):
    """The batch's inputs as the GPU gets them, read-only."""
    frames, lens, _ = source(spec.src)
    fr = reslot(frames[spec.off:spec.off + spec.n], spec.slot)
    ln = np.ascontiguousarray(lens[spec.off:spec.off + spec.n])
    ifx = ifindex_of(spec)
    for a in (fr, ln) + (() if ifx is None else (ifx,)):
        a.setflags(write=False)
    return Batch(spec, fr, ln, ifx)


@functools.lru_cache(maxsize=None)
def expected(spec, keysel, iset=ISET, partial=False, nokey=False, raw=None):
    """(words, status) the batch must give under the ctx's keysel and internal-ifindex set.
    partial: the key slots 1..6 are empty; nokey: every slot is; raw: another key table."""
    b = batch(spec)
    internal = np.isin(b.ifidx, iset) if b.ifidx is not None and len(iset) else False
    valid = None
    if partial or nokey:
        valid = keys(keysel)[2].copy()
        valid[0] &= np.uint32(~0x7E & 0xFFFFFFFF)
        if nokey:
            valid[:] = 0
    words, st = judge(b.frames, b.lens, internal, keysel, valid, raw)
    words.setflags(write=False), st.setflags(write=False)
    return words, st


def passes_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


@functools.lru_cache(maxsize=None)
def _source_passes(src, slot, ifx):
    """bool per frame of the whole source in `slot`-byte slots, under KEYSEL_ZERO and ISET."""
    frames, lens, ifidx = source(src)
    if ifx == 2:
        ifidx = np.roll(ifidx, 1)
    internal = np.isin(ifidx, ISET) if ifx else False
    words, _ = judge(reslot(frames, slot), lens, internal, 0)
    return passes_of(words, len(frames))


def ending_on_pass(src, start, n, slot=2048, ifx=1, status=True, shift=0):
    """The spec of n frames of `src` from the first offset >= start at which the last frame passes."""
    p = _source_passes(src, slot, ifx)
    off = next(o for o in range(start, len(p) - n + 1) if p[o + n - 1])
    return Spec(src, off, n, slot, ifx, status, shift)


# ---- the lists ----------------------------------------------------------------------------------

FUZZ = tuple(("fuzz", br, v6) for br, v6 in R.CASES)
RAGGED_N = (1, 63, 64, 65, 37, 1025, 4001)
SLOTS_STAGED, SLOTS_DIRECT = (2048, 256, 144), (136, 64)


def ragged():
    return [ending_on_pass(FUZZ[i % 6], 3 * i, n) for i, n in enumerate(RAGGED_N)]


def empties():
    live = [ending_on_pass(FUZZ[1], 100, 300), ending_on_pass(FUZZ[2], 900, 65), ending_on_pass(FUZZ[4], 5, 700)]
    return [EMPTY, live[0], EMPTY, EMPTY, live[1], live[2], EMPTY]


def split(count):
    """`count` non-empty batches of 1..130 frames, the sources in turn, each source's slices one
    after the other."""
    at, out = [0] * 6, []
    for i in range(count):
        n, s = 1 + (37 * i + 11 * (i // 7)) % 130, i % 6
        spec = ending_on_pass(FUZZ[s], at[s], n, slot=(256, 2048)[i % 2])
        at[s] = spec.off + n
        out.append(spec)
    return out


def corpus_batches(slot):
    """The window-edge corpus of br1 (both families) and br2 (IPv6) in batches of at most 255
    frames: every frame of it passes in 256-byte slots, so no batch reaches the 256 frames from which
    a batch must hold both verdicts."""
    out = []
    for src in (("corpus", "br1", False), ("corpus", "br1", True), ("corpus", "br2", True)):
        total = len(source(src)[0])
        out += [Spec(src, off, min(255, total - off), slot) for off in range(0, total, 255)]
    return out


def mixed():
    """Staged and direct batches in one list, a launch split at every change; the window-edge corpus
    once staged and once direct.  Slot 64 ends inside the SCION header: no frame of it passes."""
    return [ending_on_pass(FUZZ[0], 0, 700, slot=2048),
            ending_on_pass(FUZZ[1], 300, 513, slot=136),
            ending_on_pass(FUZZ[2], 50, 1000, slot=256),
            ending_on_pass(FUZZ[3], 2000, 321, slot=144),
            Spec(FUZZ[4], 100, 200, 64),
            ending_on_pass(FUZZ[5], 1500, 600, slot=256, shift=8)] + corpus_batches(256) + corpus_batches(136)


def direction():
    """Batches with an ifindex array and with NULL, with and without status; the first batch's frames
    again with another ifindex array.  A batch with an array follows one without and the other way
    round."""
    a, b = FUZZ[0], FUZZ[1]                       # br1: its internal interfaces are ISET
    return [ending_on_pass(a, 64, 1200, ifx=0),
            ending_on_pass(a, 64, 1200, ifx=1),
            ending_on_pass(b, 2000, 700, ifx=0, status=False),
            ending_on_pass(b, 1000, 900, ifx=1, status=False),
            ending_on_pass(a, 64, 1200, ifx=2),
            ending_on_pass(b, 3000, 130, ifx=0)]


LISTS = {"ragged": ragged, "empties": empties, "split33": lambda: split(33), "split70": lambda: split(70),
         "mixed": mixed, "direction": direction}


@functools.lru_cache(maxsize=None)
def specs(name):
    return tuple(LISTS[name]())


# ---- the dealing lists: frames cycled from one judged batch ---------------------------------------

CYCLE = 4001     # frames of the cycled batch: odd, so tiles 64 frames apart never start at the same frame
DEAL_SLOT = 256
TILES_PER_WAVE = 3


@functools.lru_cache(maxsize=None)
def deal_case(keysel):
    """(frames [CYCLE, 256], lens, passes bool[CYCLE]) judged once on the host."""
    frames, lens, _ = source(FUZZ[0])
    frames, lens = reslot(frames[:CYCLE], DEAL_SLOT), np.array(lens[:CYCLE])
    words, _ = judge(frames, lens, False, keysel)
    return frames, lens, passes_of(words, CYCLE)


def deal_sizes(kind, keysel, blocks):
    """Batch sizes of a dealing list for `blocks` blocks (TILES_PER_WAVE tiles per wave and more).
    small: batches of 1..9 tiles, ragged, as many as fill the blocks (several launches under a
    few blocks; the uncapped grid runs them on as many blocks as each launch's tiles fill);
    large: five ragged batches."""
    total = FD.WAVES[keysel] * blocks * TILES_PER_WAVE + 1
    if kind == "large":
        cut = [0, total // 7, total // 3, total // 3 + 1, 3 * total // 4, total]
        return [64 * (b - a) - (63, 0, 27, 1, 37)[i] for i, (a, b) in enumerate(zip(cut, cut[1:]))]
    sizes, tiles, i = [], 0, 0
    while tiles < total and len(sizes) < 4 * BATCH_MAX:
        t = 1 + (5 * i + i // 9) % 9
        sizes.append(64 * t - (63, 0, 1, 27, 62)[i % 5])
        tiles += t
        i += 1
    return sizes


def deal_words(passes, start, n):
    """The words of n frames cycled from the batch, the first being frame `start` of the cycle."""
    p = passes[(start + np.arange(n)) % CYCLE].astype(np.uint8)
    return np.packbits(np.concatenate([p, np.zeros(-n % 64, np.uint8)]), bitorder="little").view(np.uint64)
