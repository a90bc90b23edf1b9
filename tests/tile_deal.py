"""The tile dealing of k_verify_batches restated in plain Python, batch lists that stress it, and
the records those lists are made of (numpy; verdicts only from the CPU checker, tests/orc.py).

TEST INFRASTRUCTURE ONLY.

The model.  hfv_verify_batches drops empty batches and launches once per 64 non-empty ones.  A
launch numbers its batches' 64-record tiles one after the other (batch j holds global tiles
[cum[j], cum[j+1]), T = cum[nb]) and runs G = min(T, B) blocks, B the block count (one per CU, or
the test build's hfv_debug_batch_grid cap); block k verifies tiles [T*k/G, T*(k+1)/G).  Inside a
block each of the 16 waves takes tile wave-number first and then claims tiles from an LDS counter:
which wave gets which claimed tile is decided at run time, so nothing below the block range is
modelled.  (A launch also ends at 2^31 tiles; that split cannot be reached at test sizes.)

The lists.  Every size is a function of B, so that the same shapes meet 1, 2 and 3 blocks (the
capped test build, where a wave verifies a hundred tiles and more) and the real grid:

  train     a ragged large batch, 40 batches cycling n = 1, 63, 64, 65, 129, a ragged large batch
  edges     batch boundaries on block-range starts, one tile before and one tile after them, each
            ending a batch of n % 64 = 0, 1 and 63; one-record batches as the launch's first tile,
            its last tile and the last tile of a block range
  over64    150 non-empty batches (three launches) with 20 empty ones between them
  single    one batch of 64 T - 63 records
  just16, just1, just2   T = 16 B + 1 (one block has a 17th tile: one real claim), B + 1, 2 B - 1

placement() says where a list's batches fall against the block ranges; tests/test_tile_deal.py
pins it literally, so a change to a list cannot quietly move a boundary off a range start.

The records.  A base of K = 65521 (prime) generator records per key rule, one MAC bit flipped in
about half of them, judged ONCE by the CPU checker.  Record i of a list's concatenated batches is
base[(start + i) % K]; a batch holds its records in its own stride and layout (relay)."""
import collections
import functools
import zlib

import numpy as np

import orc

K = 65521
KBATCH = 64                       # kBatchMax: non-empty batches per launch
SEED = 0x711ED0A1
REMS = (0, 1, 63)                 # n % 64 of the ragged sizes
LAYOUTS = {(40, 48): (64, 72, 128), (0, 8): (24, 32, 40)}   # (inf_off, hf_off) -> strides, cycling per batch
FILLER = 0xA5                     # the bytes of a re-laid record outside its two fields
NAMES = ("train", "edges", "over64", "single", "just16", "just1", "just2")

Deal = collections.namedtuple("Deal", "index n cum T G ranges")
Place = collections.namedtuple("Place", "launches most_batches on before after partial_ends one_ends_range "
                                        "one_first one_last tiles_min tiles_max")


# ---- the model ----------------------------------------------------------------------------------

def launches(sizes):
    """[[(position in the list, n), ...], ...]: the non-empty batches, 64 per launch."""
    live = [(i, n) for i, n in enumerate(sizes) if n]
    return [live[k:k + KBATCH] for k in range(0, len(live), KBATCH)]


def deal(launch, B):
    """One launch on B blocks: cum[], T, G and every block's tile range."""
    n = [m for _, m in launch]
    cum = [0]
    for m in n:
        cum.append(cum[-1] + (m + 63) // 64)
    T = cum[-1]
    G = min(T, B)
    return Deal([i for i, _ in launch], n, cum, T, G, [(T * k // G, T * (k + 1) // G) for k in range(G)])


def placement(sizes, B):
    """Where the batches of a list fall against the block ranges, over all of its launches."""
    most, ends, one_range, tiles = 0, 0, 0, []
    at = {-1: set(), 0: set(), 1: set()}
    one_first = one_last = True
    ls = launches(sizes)
    for launch in ls:
        d = deal(launch, B)
        starts = {a for a, _ in d.ranges[1:]}
        last_tile = {d.cum[j + 1] - 1: d.n[j] for j in range(len(d.n))}    # a batch's last tile -> its n
        for a, b in d.ranges:
            most = max(most, sum(1 for j in range(len(d.n)) if d.cum[j] < b and d.cum[j + 1] > a))
            tiles.append(b - a)
            if b - 1 in last_tile and last_tile[b - 1] % 64:
                ends += 1
                one_range += last_tile[b - 1] == 1 and b != d.T
        for j in range(1, len(d.n)):               # the boundary after batch j - 1
            for off in at:
                if d.cum[j] - off in starts:
                    at[off].add(d.n[j - 1] % 64)
        one_first &= d.n[0] == 1
        one_last &= d.n[-1] == 1
    t = lambda s: tuple(sorted(s))   # noqa: E731
    return Place(len(ls), most, t(at[0]), t(at[-1]), t(at[1]), ends, one_range, one_first, one_last,
                 min(tiles), max(tiles))


# ---- the lists ----------------------------------------------------------------------------------

def n_of(tiles, rem):
    """The batch of `tiles` tiles whose size is `rem` modulo 64."""
    return 64 * tiles if rem == 0 else 64 * (tiles - 1) + rem


def big_T(B):
    """Tiles of the long lists: 2048 and more under a few blocks (128 per wave of one block),
    about 20 per block and 7 over at the real grid."""
    return max(2048, 20 * B + 7)


def train(B):
    T = big_T(B)
    first = T // 5
    return [n_of(first, 1)] + [(1, 63, 64, 65, 129)[i % 5] for i in range(40)] + [n_of(T - 64 - first, 63)]


def edges(B):
    T = big_T(B)
    G = min(T, B)
    ks = sorted({(i + 1) * G // 7 for i in range(6)}) if G >= 7 else range(1, G)
    ends = {1: 1, T - 1: 63}          # a boundary (in tiles) -> n % 64 of the batch that ends there
    for i, k in enumerate(ks):
        for d in (-1, 0, 1):          # one tile before the range start, on it, one tile after
            ends[T * k // G + d] = REMS[(d + 1 + i) % 3]
    sizes, prev = [], 0
    for c in sorted(ends):
        sizes.append(n_of(c - prev, ends[c]))
        prev = c
    return sizes + [1]


def over64(B):
    q = -(-max(17 * B, 512) // 127)   # the first launch: 127 q + 32 tiles, 17 per block and more
    live = [n_of(q * (1 + i % 3) + i % 2, REMS[i % 3]) for i in range(64)]
    live += [n_of(1 + i % 3, REMS[(i + 1) % 3]) for i in range(64, 150)]
    sizes = []
    for i, n in enumerate(live):
        if i % 7 == 3 and i < 140:
            sizes.append(0)
        sizes.append(n)
    return sizes


def single(B):
    return [64 * big_T(B) - 63]


def just_over(T):
    first = 2 * T // 5
    return [n_of(t, r) for t, r in ((first, 63), (1, 1), (T - first - 1, 1)) if t > 0]


def sizes(name, B):
    return {"train": train, "edges": edges, "over64": over64, "single": single,
            "just16": lambda b: just_over(16 * b + 1), "just1": lambda b: just_over(b + 1),
            "just2": lambda b: just_over(2 * b - 1)}[name](B)


def strides(sz, layout):
    """Batch j's stride: the layout's three, cycling."""
    return [LAYOUTS[tuple(layout)][j % 3] for j in range(len(sz))]


# ---- the records --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def keys(keysel):
    """(raw keys, hop keys, valid words): the 256-key table for KEYSEL_IFID, one key for KEYSEL_ZERO."""
    raw = orc.gen_key_table(256)
    raw = raw if keysel else raw[:16]
    return (raw,) + orc.key_table(raw)


@functools.lru_cache(maxsize=None)
def base(keysel):
    """(records u8[K, 64], passes bool[K]) in the default layout.  Read-only."""
    _, hk, valid = keys(keysel)
    recs = orc.gen_records(K, hk, keysel, seed=SEED + keysel)
    rng = np.random.default_rng(SEED + keysel)
    hit = np.nonzero(rng.random(K) < 0.5)[0]
    recs[hit, 54 + rng.integers(0, 6, len(hit))] ^= (1 << rng.integers(0, 8, len(hit))).astype(np.uint8)
    passes = judge(recs, keysel)
    recs.setflags(write=False)
    return recs, passes


def judge(recs, keysel, valid=None, stride=64, n=None):
    """The CPU checker's verdicts, bool[n], of records with the fields at the default offsets."""
    _, hk, v = keys(keysel)
    n = len(recs) if n is None else n
    words = orc.verify_records(recs, hk, v if valid is None else valid, keysel, stride=stride, n=n)
    p = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    p.setflags(write=False)
    return p


def relay(recs, layout, stride):
    """Default-layout records as records of another stride and layout: the two fields at their
    offsets, FILLER everywhere else."""
    out = np.full((len(recs), stride), FILLER, dtype=np.uint8)
    out[:, layout[0]:layout[0] + 8] = recs[:, 40:48]
    out[:, layout[1]:layout[1] + 12] = recs[:, 48:60]
    return out


def start(name):
    """The list's seeded start in the base."""
    return int(np.random.default_rng([SEED, zlib.crc32(name.encode())]).integers(K))


def index(name, sz):
    """Base index of every record of the list's concatenated batches."""
    return (start(name) + np.arange(sum(sz))) % K


def words(passes, n):
    """The u64 verdict words of n verdicts; bits at and past n are 0."""
    p = np.concatenate([np.asarray(passes[:n], dtype=np.uint8), np.zeros(-n % 64, dtype=np.uint8)])
    return np.packbits(p, bitorder="little").view(np.uint64)


def expected(name, sz, passes):
    """Per batch the expected verdict words (None for an empty batch)."""
    want, off = passes[index(name, sz)], 0
    out = []
    for n in sz:
        out.append(words(want[off:off + n], n) if n else None)
        off += n
    return out


def full_tile_words(name, sz, passes):
    """The expected words of every full tile of the list."""
    full = [w[:n // 64] for w, n in zip(expected(name, sz, passes), sz) if n >= 64]
    return np.concatenate(full) if full else np.zeros(0, dtype=np.uint64)


def assert_no_word_can_stand_in(name, sz, passes):
    """All full tiles of the list expect pairwise distinct words, none 0 or all ones: a word
    taken from any other tile, a dropped word (the pre-fill) or a zeroed one cannot pass."""
    full = full_tile_words(name, sz, passes)
    assert len(np.unique(full)) == len(full), (name, "two full tiles expect the same word")
    assert not (full == 0).any() and not (full == np.uint64(0xFFFFFFFFFFFFFFFF)).any(), name


# ---- frames -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def frame_template():
    """(frame bytes, InfoField offset, HopField offset): a minimal valid SCION frame, one segment
    of one hop field, whose two fields a base record's replace."""
    import scion_hfv as hfv
    from scion_hfv import packets as P
    from scion_hfv import topology as TP
    path = P.Path([P.InfoField(True)], [P.HopField(1, 2)], [1])
    raw = TP.encaps(1, 2)[0].frame(P.scion_header(path.pack()))
    status, inf_off, hf_off = hfv.frame_locate(raw)
    assert status == 0
    return raw, inf_off, hf_off


def frames(recs):
    """(frames u8[n, slot], length): every record's two fields in the template frame."""
    raw, inf_off, hf_off = frame_template()
    out = np.zeros((len(recs), -(-len(raw) // 8) * 8), dtype=np.uint8)
    out[:, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    out[:, inf_off:inf_off + 8] = recs[:, 40:48]
    out[:, hf_off:hf_off + 12] = recs[:, 48:60]
    return out, len(raw)
