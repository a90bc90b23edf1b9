"""The grid and round model of the kernels in csrc/hfv_aux_kernels.hip and the corpora that hold them
on every round of their grid-stride loops, every tail and every edge of the key validity words
(tests/test_aux_edges.py holds this module to itself, to the header and to the CPU checker;
tests/test_gpu_aux_edges.py runs the kernels on it).  No GPU imports.

Three kernels loop: k_macinputs (hfv_verify_macinputs, hfv_cmac_tags) deals tiles of 64 items to
waves, wave w of W takes tiles w, w + W, ...; k_count_verdicts (hfv_verdict_counters) and
k_gen_records (hfv_gen_records) deal items to threads, thread p of P takes items p, p + P, ....
All three run blocks of 512 threads, so with a grid of G blocks a round holds C = 512 G items.  The
launchers cap G at 2 blocks per CU (k_macinputs, k_gen_records) or 1 (k_count_verdicts); the test
build's hfv_debug_aux_grid caps it further, at B blocks.

Everything expected here comes from the CPU checker (tests/orc.py), is built once and is read-only."""
import functools

import numpy as np

import key_tables as KT
import orc

BLOCK = 512                       # kBlockAux, kCountBlock
WAVES = BLOCK // 64
KERNELS = ("macinputs", "count", "gen")
PER_CU = {"macinputs": 2, "count": 1, "gen": 2}
CAPS = (1, 2, 3)
U64 = (1 << 64) - 1


def _ro(a):
    a.setflags(write=False)
    return a


# ---- a. grid and round model ----------------------------------------------------------------

def grid_for(n, block, num_cus, per_cu):
    """csrc/hfv_verify_dev.h, in plain integers."""
    tiles = (n + 63) // 64
    blocks = (tiles + block // 64 - 1) // (block // 64)
    cap = num_cus * (per_cu if per_cu > 0 else 1)
    return max(1, min(blocks, cap))


def gen_grid(n, num_cus):
    """launch_gen_records' own rule."""
    blocks = (n + BLOCK - 1) // BLOCK
    return max(1, min(blocks, 2 * num_cus))


def grid(kernel, n, num_cus, cap=0):
    """Blocks of the launch for n items; cap: hfv_debug_aux_grid (0: none)."""
    g = gen_grid(n, num_cus) if kernel == "gen" else grid_for(n, BLOCK, num_cus, PER_CU[kernel])
    return min(g, cap) if cap else g


def where(kernel, i, G):
    """Item i on a grid of G blocks -> (block, wave of the block, round from 0, lane)."""
    if kernel == "macinputs":
        t, W = i // 64, G * WAVES
        return (t % W) // WAVES, (t % W) % WAVES, t // W, i % 64
    p = i % (G * BLOCK)
    return p // BLOCK, (p % BLOCK) // 64, i // (G * BLOCK), p % 64


def round_items(G):
    return BLOCK * G


def rounds(kernel, n, G):
    """Rounds the busiest wave runs."""
    return where(kernel, n - 1, G)[2] + 1 if kernel != "macinputs" else -(-((n + 63) // 64) // (G * WAVES))


def placement(kernel, n, num_cus, cap=0):
    """(rounds of the busiest wave, a partial tile lies in a round >= 2)"""
    G = grid(kernel, n, num_cus, cap)
    return rounds(kernel, n, G), bool(n % 64) and where(kernel, n - 1, G)[2] >= 1


# ---- b, c. sizes ----------------------------------------------------------------------------

def sizes(B):
    C = round_items(B)
    return (1, 63, 64, 65, C - 1, C, C + 1, C + 63, C + 64, C + 65, 2 * C, 2 * C + 1, 5 * C + 3 * 64 + 17)


N_CAPPED = max(sizes(max(CAPS)))   # 7889: the capped corpora are prefixes of one of this length


def n_real(kernel, num_cus):
    return 2 * round_items(PER_CU[kernel] * num_cus) + 3 * 64 + 17


# ---- d. verdict design -----------------------------------------------------------------------

MIX_SEED = 0xA0C5ED6E5EED0001


def mix(t):
    """64-bit mix of t (splitmix64 at counter t), vectorised."""
    t = np.asarray(t, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(MIX_SEED) + (t + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def want_words(n):
    """The wanted bitmap of n items: word t is mix(t), bits at and past n are zero."""
    w = mix(np.arange((n + 63) // 64))
    if n % 64:
        w[-1] &= np.uint64((1 << (n % 64)) - 1)
    return w


def want_bool(n):
    return np.unpackbits(want_words(n).view(np.uint8), bitorder="little")[:n].astype(bool)


pack = KT.pack_bits   # bool[n] -> u64 words, bit i of word i / 64


def mac48(tags):
    """Tag bytes 0..5 as a little-endian u64 (xdp.c:89: *(u64 *)mac.w & 0xffffffffffff)."""
    return np.frombuffer(np.pad(tags[:, :6], ((0, 0), (0, 2))).tobytes(), dtype=np.uint64).copy()


@functools.lru_cache(maxsize=None)
def full_table():
    """(raw keys, hop_keys, valid) of the full 256-key table (key_tables' table A)."""
    return KT.tables()["A"]


@functools.lru_cache(maxsize=4)
def mac_corpus(n):
    """{use_index: (macinput u8[n, 16], key_index u8[n], tags u8[n, 16], expected u64[n])} under the
    full table: random macinputs, a random slot each; without an index every item is slot 0's.
    expected[i] is the true MAC where bit i of the wanted bitmap is set, else the true MAC with bit
    i % 48 flipped.  A prefix of the corpus is the corpus of that size."""
    rng = np.random.default_rng(0xA0E)
    mi = _ro(rng.integers(0, 256, size=(n, 16), dtype=np.uint8))
    kidx = _ro(rng.integers(0, 256, size=n, dtype=np.uint8))
    _, hk, valid = full_table()
    flip = np.where(want_bool(n), np.uint64(0), np.uint64(1) << (np.arange(n, dtype=np.uint64) % np.uint64(48)))
    out = {}
    for use in (False, True):
        tags = _ro(orc.cmac16_bulk(mi, hk, valid, kidx if use else None))
        out[use] = (mi, kidx, tags, _ro(mac48(tags) ^ flip))
    return out


# ---- e, f. slot edges and the five classes of expected ----------------------------------------

E_VALID = (0, 31, 32, 63, 64, 255)
EDGE_TABLES = {"E": frozenset(E_VALID), "E'": frozenset(range(256)) - frozenset(E_VALID)}
EDGE_SLOTS = tuple(s for s in range(256) if s % 32 in (0, 1, 30, 31))   # 255 is among them
CLASSES = ("true", "flip", "high", "zero", "stale")


def stale_slot(s, valid):
    """The removed slot whose old key class 5 takes: s itself where s was removed, else the next
    removed slot above it (cyclic)."""
    while s in valid:
        s = (s + 1) % 256
    return s


@functools.lru_cache(maxsize=None)
def edge_corpus(name):
    """(macinput u8[n, 16], key_index u8[n], expected u64[n], class index u8[n], want bool[n],
    tags u8[n, 16], true MAC u64[n]) for table E or E': the ctx holds the full table with every slot outside the
    valid set removed.  Per visited slot 20 entries, each with a macinput of its own: the true MAC (under the key the full table has
    in that slot), one flipped bit, the true MAC with each of bits 48..63 set, zero, and the true
    MAC under the old key of a removed slot.  Only a true MAC in a valid slot passes."""
    valid = EDGE_TABLES[name]
    raw, hk, _ = full_table()
    rng = np.random.default_rng(0xED6E + len(valid))
    ks, cls, exp = [], [], []
    n = 20 * len(EDGE_SLOTS)
    mi = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    for j, s in enumerate(EDGE_SLOTS):
        ks += [s] * 20
        cls += [0, 1] + [2] * 16 + [3, 4]
    ks = np.array(ks, dtype=np.uint8)
    true = mac48(orc.cmac16_bulk(mi, hk, np.full(8, 0xffffffff, dtype=np.uint32), ks))
    other = np.array([stale_slot(int(s), valid) for s in ks], dtype=np.uint8)
    stale = mac48(orc.cmac16_bulk(mi, hk, np.full(8, 0xffffffff, dtype=np.uint32), other))
    for i in range(n):
        k, c = i % 20, cls[i]
        exp.append(int(true[i]) if c == 0 else int(true[i]) ^ (1 << ((i // 20 * 7 + 3) % 48)) if c == 1 else
                   int(true[i]) | (1 << (48 + k - 2)) if c == 2 else 0 if c == 3 else int(stale[i]))
    cls = np.array(cls, dtype=np.uint8)
    want = np.array([c == 0 and int(s) in valid for c, s in zip(cls, ks)])
    vw = valid_words(valid)
    return (_ro(mi), _ro(ks), _ro(np.array(exp, dtype=np.uint64)), _ro(cls), _ro(want),
            _ro(orc.cmac16_bulk(mi, hk, vw, ks)), _ro(true))


def valid_words(valid):
    w = np.zeros(8, dtype=np.uint32)
    for s in valid:
        w[s >> 5] |= np.uint32(1 << (s & 31))
    return w


# ---- g. generator cases ----------------------------------------------------------------------

GEN_STRIDES = (64, 80, 128)
GEN_SEED = orc.SEED_RECORDS + 0xA0


def gen_firsts(n):
    """Every window [first, first + n) crosses its edge: 2^30 (4 i past 2^32), 2^32 (the payload
    word), 2^62 (4 i past 2^64) and 2^64 (i itself wraps)."""
    return (0, (1 << 30) - 3, (1 << 32) - 3, (1 << 62) - 3, ((1 << 64) - n) & U64)


def gen_pass_rule(n, first, seed=GEN_SEED):
    """orc.expected_pass_rule with the index wrapping at 2^64 as the generators' own u64 does."""
    with np.errstate(over="ignore"):
        i = np.uint64(first) + np.arange(n, dtype=np.uint64)
        z = np.uint64(seed) + (np.uint64(4) * i + np.uint64(3)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(15)) != 0


@functools.lru_cache(maxsize=64)
def gen_want(n, first, keysel):
    """The n records of index first.. under the full table (the CPU twin, orc_gen_records)."""
    return _ro(orc.gen_records(n, full_table()[1], keysel, seed=GEN_SEED, first_index=first))


# ---- h. counter cases ------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def count_records(n):
    """n generated records (KEYSEL_IFID) whose key slots cover 0..255 with both Cons values: the
    generator draws interfaces 1..255, so every 97th record's AS-ingress IFID byte is rewritten
    to 0.  A prefix is the corpus of that size."""
    recs = orc.gen_records(n, full_table()[1], 1, seed=GEN_SEED + 1)
    i = np.arange(0, n, 97)
    cons = recs[i, 40] & 1
    recs[i, np.where(cons, 51, 53)] = 0
    return _ro(recs)


def count_slots(recs):
    return np.where(recs[:, 40] & 1, recs[:, 51], recs[:, 53]).astype(np.int64)


def count_preload():
    """counters u64[256, 2] before the call: most 0, some 2^32 - 3 (the 32-bit LDS bin added to it
    carries out of bit 31), one 2^63."""
    c = np.zeros((256, 2), dtype=np.uint64)
    for s in (0, 1, 31, 32, 128, 255):
        c[s, 0] = (1 << 32) - 3
    for s in (0, 7, 254):
        c[s, 1] = (1 << 32) - 3
    c[200, 0] = 1 << 63
    return c


def count_want(recs, n, pre):
    """pre + [verified, INVALID_HF] per slot, the bitmap being want_words(n)."""
    out = pre.copy()
    np.add.at(out, (count_slots(recs[:n]), (~want_bool(n)).astype(np.int64)), np.uint64(1))
    return out


def compact(recs):
    """The records in the layout (0, 8) with a 24-byte stride."""
    c = np.zeros((len(recs), 24), dtype=np.uint8)
    c[:, 0:8] = recs[:, 40:48]
    c[:, 8:20] = recs[:, 48:60]
    return c


# ---- i. expansion keys -----------------------------------------------------------------------

CARRY_NAMES = ("msb of L", "into word 0", "into word 1", "into word 2")
CARRY_SEED = 0xCA55E77E


def carries(key):
    """The four carry bits of the K1 doubling for a raw key: the msb of L = E_K(0^128) and the bits
    that move from big-endian word 1, 2, 3 of L into word 0, 1, 2."""
    hk = orc.hop_key(key)
    L = np.zeros(16, dtype=np.uint8)
    z = np.zeros(16, dtype=np.uint8)
    orc.oracle().orc_cypher(orc._vp(z), hk[:176], orc._vp(L))
    return tuple(int(L[4 * w]) >> 7 for w in range(4))


def carry_search():
    """{(position, bit): the first key of the seeded stream with that carry bit}"""
    found, j = {}, 0
    while len(found) < 8:
        a, b = orc.oracle().orc_splitmix_at(CARRY_SEED, 2 * j), orc.oracle().orc_splitmix_at(CARRY_SEED, 2 * j + 1)
        key = int(a).to_bytes(8, "little") + int(b).to_bytes(8, "little")
        for p, bit in enumerate(carries(key)):
            found.setdefault((p, bit), key)
        j += 1
    return found


# (position, bit) -> key, as carry_search finds them (tests/test_aux_edges.py asserts it)
CARRY_KEYS = {
    (0, 0): "4949a3a92fab0227fae64f84d7f85d56", (0, 1): "3cd0da93488d6c9fa43256914cacf50a",
    (1, 0): "02347373951612303f464a8c18c04660", (1, 1): "4949a3a92fab0227fae64f84d7f85d56",
    (2, 0): "4949a3a92fab0227fae64f84d7f85d56", (2, 1): "8a0cf0d4baac36b034143417f340c242",
    (3, 0): "4949a3a92fab0227fae64f84d7f85d56", (3, 1): "02347373951612303f464a8c18c04660",
}

EXPAND_N = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def expand_keys():
    """(raw keys u8[257, 16], hop_keys u8[257, 192]): the all-zero key, the all-ones key, the carry
    keys, then generated keys."""
    head = [bytes(16), b"\xff" * 16] + [bytes.fromhex(CARRY_KEYS[k]) for k in sorted(CARRY_KEYS)]
    raw = b"".join(head) + orc.gen_key_table(max(EXPAND_N) - len(head), orc.SEED_KEYS + 7)
    hk = b"".join(orc.hop_key(raw[16 * k:16 * k + 16]) for k in range(max(EXPAND_N)))
    return (_ro(np.frombuffer(raw, dtype=np.uint8).reshape(-1, 16).copy()),
            _ro(np.frombuffer(hk, dtype=np.uint8).reshape(-1, 192).copy()))
