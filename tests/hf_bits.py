"""A corpus of PASSING hop-field records with every don't-care bit set, and the rule that says
which of them pass (numpy; only AES-CMAC comes from the CPU checker, tests/orc.py).

TEST INFRASTRUCTURE ONLY.  The record generators (k_gen_records, orc_gen_records) write
hf[0] = 0, inf[0] in {0, 1}, inf[1] = 0, IFIDs in [1, 255] and a fixed header, and corrupt only
MAC bits; the random records of the other tests fail everywhere.  Here:

* 2048 base records per key rule: all 64 bytes random, then the fields fixed up so that the MAC
  is right.  The MAC input is built in this file from the reference text
  (br/src/bpf/path_processing.h:45-53: beta, ts, exp, ingress, egress into the zeroed struct
  macinput of include/bpf/scion.h; path_processing.h:73-77: beta = SegID, xor MAC[0:2] when
  Cons is clear), the key slot by xdp.c:151-157 (Cons ? ConsIngress : ConsEgress, low byte).
* For 8 base records per key rule (4 Cons, 4 non-Cons) every single-bit flip of the record.

The rule: a base record passes; a variant passes iff its flipped bit is outside SENS = bit 0 of
INF byte 0, INF bytes 2..7 and HF bytes 1..11 (137 bits).  Under a partial key table (only the
even slots, KEYSEL_IFID) a record passes iff it passes the full-table rule and its slot is even.

The same records are laid out as (inf_off, hf_off, stride) = (40, 48, 64), (0, 8, 24) and
(8, 16, 72); the variants flip every bit of the stride and SENS moves with the offsets.

tests/test_hf_bits.py holds the rule to the CPU checker, to the reference build and to the
reference's recorded bitmaps (tests/golden/hf_bits.npz); tests/test_gpu_hf_bits.py holds the
kernels to the rule.
"""
import collections
import functools
import hashlib

import numpy as np

import orc

SEED = 0x5C10B175
LAYOUTS = ((40, 48, 64), (0, 8, 24), (8, 16, 72))
NBASE = 2048
SLOT_RECORDS = 1536                 # records [0, 1536): Cons = i & 1, slot = (i >> 1) & 0xff
VAR_BASES = (0, 1, 514, 515, 1536, 1537, 1568, 1569)   # i & 1 = Cons: 4 and 4
SENS_BITS = 137

Corpus = collections.namedtuple("Corpus", "recs passes keysel layout nbase")


def splitmix(seed, count, start=0):
    """orc_splitmix_at(seed, start + j) for j < count (hfv_oracle.c), as orc.expected_pass_rule
    states it."""
    k = np.arange(start, start + count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (k + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def random_bytes(seed, shape):
    n = int(np.prod(shape))
    return splitmix(seed, (n + 7) // 8).astype("<u8").view(np.uint8)[:n].reshape(shape).copy()


@functools.lru_cache(maxsize=None)
def raw_keys():
    return orc.gen_key_table(256)


def fields(recs, layout):
    """(inf[n, 8], hf[n, 12]) views of recs[n, stride]."""
    inf_off, hf_off, _ = layout
    return recs[:, inf_off:inf_off + 8], recs[:, hf_off:hf_off + 12]


def macinput_block(beta, ts, exp, ingress, egress):
    """struct macinput as defer_verify_hop_field fills it (path_processing.h:45-53): zeroed, then
    beta (network order), ts, exp, ingress, egress, the last three as they stand on the wire."""
    mi = np.zeros((len(beta), 16), dtype=np.uint8)
    mi[:, 2] = beta >> 8
    mi[:, 3] = beta & 0xff
    mi[:, 4:8] = ts
    mi[:, 9] = exp
    mi[:, 10:12] = ingress
    mi[:, 12:14] = egress
    return mi


def macinputs(recs, layout):
    """(macinput u8[n, 16], expected u64[n]) of wire records, by scion_as_ingress
    (path_processing.h:73-77): beta = ntohs(SegID), xor'ed with mac[0] << 8 | mac[1] when the
    Cons flag (bit 0 of the InfoField flags) is clear; expected = the 6 MAC bytes, little-endian."""
    inf, hf = fields(recs, layout)
    beta = inf[:, 2].astype(np.uint16) << 8 | inf[:, 3]
    noncons = (inf[:, 0] & 1) == 0
    beta = np.where(noncons, beta ^ (hf[:, 6].astype(np.uint16) << 8 | hf[:, 7]), beta)
    mi = macinput_block(beta, inf[:, 4:8], hf[:, 1], hf[:, 2:4], hf[:, 4:6])
    expected = np.zeros(len(recs), dtype=np.uint64)
    for j in range(6):
        expected |= hf[:, 6 + j].astype(np.uint64) << np.uint64(8 * j)
    return mi, expected


def selecting_ifid(recs, layout):
    """xdp.c:151-157: Cons ? hf->ingress : hf->egress, all 16 bits (host order)."""
    inf, hf = fields(recs, layout)
    ing = hf[:, 2].astype(np.uint16) << 8 | hf[:, 3]
    eg = hf[:, 4].astype(np.uint16) << 8 | hf[:, 5]
    return np.where(inf[:, 0] & 1, ing, eg)


def other_ifid(recs, layout):
    inf, hf = fields(recs, layout)
    ing = hf[:, 2].astype(np.uint16) << 8 | hf[:, 3]
    eg = hf[:, 4].astype(np.uint16) << 8 | hf[:, 5]
    return np.where(inf[:, 0] & 1, eg, ing)


def slots(recs, layout):
    """The KEYSEL_IFID key slot: the low byte of the selecting IFID."""
    return (selecting_ifid(recs, layout) & 0xff).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _base(keysel):
    """(body u8[NBASE, 64] of random bytes, inf u8[NBASE, 8], hf u8[NBASE, 12]) with a right MAC."""
    body = random_bytes(SEED + 16 * keysel, (NBASE, 64))
    inf, hf = body[:, 40:48].copy(), body[:, 48:60].copy()
    i = np.arange(NBASE)
    cons = (i & 1).astype(np.uint8)
    inf[:, 0] = (inf[:, 0] & 0xfe) | cons
    ing = hf[:, 2].astype(np.uint16) << 8 | hf[:, 3]
    eg = hf[:, 4].astype(np.uint16) << 8 | hf[:, 5]
    sel, oth = np.where(cons, ing, eg), np.where(cons, eg, ing)
    # [0, 1536): every (slot, Cons) pair three times; [0, 512) plain IFIDs below 256, [512, 1024)
    # a high byte that is never 0, [1024, 1536) a random high byte
    sel = np.where(i < SLOT_RECORDS, (sel & 0xff00) | ((i >> 1) & 0xff), sel)
    sel = np.where(i < 512, sel & 0xff, sel)
    sel = np.where((i >= 512) & (i < 1024) & (sel >> 8 == 0), sel | 0x100, sel)
    # [1536, 1568): selecting IFID 0; [1568, 1600): the other IFID 0; [1600, 2048): both random
    sel = np.where((i >= 1536) & (i < 1568), 0, sel).astype(np.uint16)
    oth = np.where((i >= 1568) & (i < 1600), 0, oth).astype(np.uint16)
    ing, eg = np.where(cons, sel, oth), np.where(cons, oth, sel)
    hf[:, 2], hf[:, 3], hf[:, 4], hf[:, 5] = ing >> 8, ing & 0xff, eg >> 8, eg & 0xff
    beta = inf[:, 2].astype(np.uint16) << 8 | inf[:, 3]
    raw = raw_keys()
    for r in range(NBASE):
        slot = int(sel[r]) & 0xff if keysel else 0
        while True:
            mi = macinput_block(beta[r:r + 1], inf[r:r + 1, 4:8], hf[r:r + 1, 1], hf[r:r + 1, 2:4], hf[r:r + 1, 4:6])
            tag = orc.cmac(mi.tobytes(), raw[16 * slot:16 * slot + 16])
            if tag[0] or tag[1]:        # mac[0:2] != 0: flipping Cons must change beta
                break
            inf[r, 7] = (int(inf[r, 7]) + 1) & 0xff   # another timestamp
        hf[r, 6:12] = np.frombuffer(tag[:6], dtype=np.uint8)
        seg = int(beta[r]) if cons[r] else int(beta[r]) ^ (tag[0] << 8 | tag[1])
        inf[r, 2], inf[r, 3] = seg >> 8, seg & 0xff
    return body, inf, hf


def sens(layout):
    """bool[8 * stride]: the bits of a record that the verdict depends on."""
    inf_off, hf_off, stride = layout
    s = np.zeros((stride, 8), dtype=bool)
    s[inf_off, 0] = True                 # Cons
    s[inf_off + 2:inf_off + 8] = True    # SegID, timestamp
    s[hf_off + 1:hf_off + 12] = True     # ExpTime, ConsIngress, ConsEgress, MAC
    return s.reshape(-1)


@functools.lru_cache(maxsize=None)
def corpus(keysel, layout=LAYOUTS[0]):
    """Corpus(recs u8[n, stride], passes bool[n], ...): the base records, then for each of
    VAR_BASES its 8 * stride single-bit flips (bit b: byte b >> 3, bit b & 7).  Read-only."""
    layout = tuple(layout)
    inf_off, hf_off, stride = layout
    body, inf, hf = _base(keysel)
    base = body.copy() if layout == LAYOUTS[0] else random_bytes(SEED + 16 * keysel + 1 + LAYOUTS.index(layout), (NBASE, stride))
    base[:, inf_off:inf_off + 8] = inf
    base[:, hf_off:hf_off + 12] = hf
    nb = 8 * stride
    b = np.arange(nb)
    blocks = []
    for r in VAR_BASES:
        v = np.repeat(base[r:r + 1], nb, axis=0)
        v[b, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
        blocks.append(v)
    recs = np.concatenate([base] + blocks)
    passes = np.concatenate([np.ones(NBASE, dtype=bool)] + [~sens(layout)] * len(VAR_BASES))
    recs.setflags(write=False)
    passes.setflags(write=False)
    return Corpus(recs, passes, keysel, layout, NBASE)


def partial_valid():
    """The valid words of a key table with only the even slots installed."""
    return np.full(8, 0x55555555, dtype=np.uint32)


def partial_passes(c):
    """The rule under KEYSEL_IFID with only the even slots installed."""
    return c.passes & (slots(c.recs, c.layout) % 2 == 0)


def bitmap(passes, n=None):
    """The u64 verdict words of passes[:n]; bits at and past n are 0."""
    p = np.asarray(passes[:n], dtype=np.uint8)
    p = np.concatenate([p, np.zeros(-len(p) % 64, dtype=np.uint8)])
    return np.packbits(p, bitorder="little").view(np.uint64)


def sha256(c):
    return hashlib.sha256(c.recs.tobytes()).digest()


def at_default_offsets(recs, layout):
    """recs[n, stride] as a byte array whose element 40 + i * stride is record i's InfoField and
    48 + i * stride its HopField, so that a verifier with the fixed offsets 40/48 (the CPU
    checker, the reference build) reads the layout's records when given (array, stride, n)."""
    inf_off, hf_off, stride = layout
    assert hf_off - inf_off == 8 and inf_off <= 40
    buf = np.zeros(40 + recs.size + 64, dtype=np.uint8)
    buf[40:40 + recs.size] = recs.reshape(-1)
    return buf[inf_off:]
