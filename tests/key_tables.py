"""Three 256-key tables and one record corpus that tells them apart, for the tests of key-table
publication (tests/test_gpu_key_publish.py and the keysel 1 legs of the key-change tests in
test_gpu_parity.py / test_gpu_service.py).

Tables A, B, C are gen_key_table(256, SEED_KEYS + i).  The corpus is 1500 records generated under
each table (KEYSEL_IFID), shuffled together: under table X only records generated for X can pass,
so a batch verified under another table than the one it was launched with differs from the right
answer in well over half of its bits, spread over (nearly) every key slot.  tests/test_key_tables.py
holds those properties on the CPU, so the GPU tests cannot become vacuous.

Everything here comes from the CPU checker (tests/orc.py), is built once and is read-only."""
import functools

import numpy as np

import orc

NAMES = ("A", "B", "C")
PER_TABLE = 1500
N = PER_TABLE * len(NAMES)
# verify_batches: the corpus cut here (an empty batch, one-record batches, a tile and a tile + 1)
CUTS = (0, 1, 1, 64, 65, 700, N)
GEN_N = 5000          # gen_records leg: records generated on the device under each table
TAG_SAMPLE = 256      # cmac_tags leg: records whose full tags are compared


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tables():
    """{name: (raw_keys bytes[4096], hop_keys u8[256 * 192], valid u32[8])}"""
    out = {}
    for i, name in enumerate(NAMES):
        raw = orc.gen_key_table(256, orc.SEED_KEYS + i)
        hk, valid = orc.key_table(raw)
        out[name] = (raw, _ro(hk), _ro(valid))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """(records u8[N, 64], origin u8[N]): origin[i] is the index of the table record i was made for."""
    parts, origin = [], []
    for i, name in enumerate(NAMES):
        parts.append(orc.gen_records(PER_TABLE, tables()[name][1], 1, seed=orc.SEED_RECORDS + i))
        origin.append(np.full(PER_TABLE, i, dtype=np.uint8))
    perm = np.random.default_rng(1).permutation(N)
    return _ro(np.concatenate(parts)[perm].copy()), _ro(np.concatenate(origin)[perm].copy())


@functools.lru_cache(maxsize=None)
def want():
    """{name: verdict bitmap u64[(N + 63) // 64] of the corpus under that table (KEYSEL_IFID)}"""
    recs, _ = corpus()
    return {name: _ro(orc.verify_records(recs, tables()[name][1], tables()[name][2], 1)) for name in NAMES}


@functools.lru_cache(maxsize=None)
def want_bool():
    return {name: _ro(np.unpackbits(want()[name].view(np.uint8), bitorder="little")[:N].astype(bool))
            for name in NAMES}


def slots():
    """Key slot (AS-ingress IFID & 0xff) of every corpus record, as tests/test_gpu_parity.py reads it."""
    recs, _ = corpus()
    return np.where(recs[:, 40] & 1, recs[:, 51], recs[:, 53])


@functools.lru_cache(maxsize=None)
def macinputs():
    """(macinput u8[N, 16], expected u64[N], key_index u8[N]) of the corpus, taken as
    test_golden_tags_and_verdicts takes them."""
    recs, _ = corpus()
    mi, _, kidx = orc.macinputs_from_records(recs)
    expected = np.frombuffer(np.pad(recs[:, 54:60], ((0, 0), (0, 2))).tobytes(), dtype=np.uint64).copy()
    return _ro(mi), _ro(expected), _ro(kidx)


def pack_bits(b):
    """bool[n] -> u64[(n + 63) // 64], bit i of word i / 64 (the kernels' bitmap layout)."""
    n = len(b)
    padded = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    padded[:n] = b
    return np.packbits(padded, bitorder="little").view(np.uint64)


@functools.lru_cache(maxsize=None)
def want_batches():
    """{name: [bitmap of corpus[CUTS[k]:CUTS[k + 1]] under that table, ...]}"""
    return {name: [_ro(pack_bits(want_bool()[name][a:b])) for a, b in zip(CUTS[:-1], CUTS[1:])] for name in NAMES}


@functools.lru_cache(maxsize=None)
def tag_sample():
    """Indices of TAG_SAMPLE records spread over the whole corpus (every third of it included)."""
    return _ro(np.linspace(0, N - 1, TAG_SAMPLE).astype(np.int64))


@functools.lru_cache(maxsize=None)
def want_tags():
    """{name: full CMAC tags u8[TAG_SAMPLE, 16] of the sampled macinputs under that table's keys}"""
    mi, _, kidx = macinputs()
    out = {}
    for name in NAMES:
        raw = tables()[name][0]
        out[name] = _ro(np.array([np.frombuffer(orc.cmac(mi[i].tobytes(), raw[16 * int(kidx[i]):16 * int(kidx[i]) + 16]),
                                                dtype=np.uint8) for i in tag_sample()]))
    return out


@functools.lru_cache(maxsize=None)
def want_gen():
    """{name: the GEN_N records the generator writes under that table (KEYSEL_IFID, SEED_RECORDS)}"""
    return {name: _ro(orc.gen_records(GEN_N, tables()[name][1], 1)) for name in NAMES}
