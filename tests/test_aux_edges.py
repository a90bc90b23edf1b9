"""tests/aux_edges.py held to itself, to csrc/hfv_verify_dev.h and to the CPU checker (no GPU): the
grid model agrees with grid_for compiled from the header and with a table of literal values, every
size's placement is pinned, no verdict word can stand in for another, the checker's own verdicts
agree with the designed bitmaps (and the reference's aes_cmac with the checker, where it was built),
the generator cases satisfy the pass rule, every carry class of the K1 doubling has its key, and
the hook exists in the test build only -- so that tests/test_gpu_aux_edges.py cannot pass by accident."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import aux_edges as AE
import orc
import scion_hfv as hfv

CUS = 256                         # the MI355X's CUs: the real grid of the GPU legs
CSRC = os.path.join(orc.ROOT, "scion-xdp-br_amd", "csrc")

# (n, block, num_cus, per_cu) -> grid_for: the caps' edges of the three launchers on 256 CUs (a second
# round starts past 262 144 items, 131 072 for the counters), another CU count, per_cu 0
GRID_FOR = {
    (0, 512, 256, 2): 1, (1, 512, 256, 2): 1, (512, 512, 256, 2): 1, (513, 512, 256, 2): 2,
    (262144, 512, 256, 2): 512, (262145, 512, 256, 2): 512, (131072, 512, 256, 1): 256,
    (131073, 512, 256, 1): 256, (1 << 40, 512, 304, 2): 608, (65, 1024, 256, 0): 1,
}

# per size of AE.sizes(B), in its order: (rounds the busiest wave runs, a partial tile lies in a round
# >= 2).  One round holds 512 B items under every one of the three kernels, so the row is the same for
# all nine (kernel, B); the real grid's sizes follow.
ROW = ((1, False), (1, False), (1, False), (1, False), (1, False), (1, False), (2, True), (2, True), (2, False),
       (2, True), (2, False), (3, True), (6, True))
PLACEMENT = {(k, B): ROW for k in AE.KERNELS for B in AE.CAPS}
REAL = {"macinputs": (524497, 512, (3, True)), "count": (262353, 256, (3, True)), "gen": (524497, 512, (3, True))}

HOST_SRC = r"""
#include <stdio.h>
#include "hfv_verify_dev.h"
int main()
{
    static const unsigned long long Q[][4] = {%s};
    for (auto &q : Q) printf("%%u\n", hfv::grid_for(q[0], (int)q[1], (int)q[2], (int)q[3]));
    return 0;
}
"""


def test_model_agrees_with_literal_values():
    assert {q: AE.grid_for(*q) for q in GRID_FOR} == GRID_FOR
    assert [AE.gen_grid(n, 256) for n in (0, 1, 512, 513, 262144, 262145, 1 << 40)] == [1, 1, 1, 2, 512, 512, 512]
    assert [AE.grid("count", 10 ** 6, 256, cap) for cap in (0, 1, 2, 3, 300)] == [256, 1, 2, 3, 256]
    assert AE.grid("macinputs", 65, 256, 3) == 1      # the cap never raises a grid


def test_model_agrees_with_the_header(tmp_path):
    """grid_for from csrc/hfv_verify_dev.h, compiled for the host only, over the literal queries and
    every size the GPU legs launch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc builds this project; it compiles the header for the host here"
    qs = list(GRID_FOR)
    for k in ("macinputs", "count"):
        for B in AE.CAPS:
            qs += [(n, AE.BLOCK, CUS, AE.PER_CU[k]) for n in AE.sizes(B)]
        qs.append((AE.n_real(k, CUS), AE.BLOCK, CUS, AE.PER_CU[k]))
    src = tmp_path / "grid_for.hip"
    src.write_text(HOST_SRC % ", ".join("{%dull, %d, %d, %d}" % q for q in qs))
    exe = tmp_path / "grid_for"
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [AE.grid_for(*q) for q in qs]


def test_placement_table():
    got = {(k, B): tuple(AE.placement(k, n, CUS, B) for n in AE.sizes(B)) for k in AE.KERNELS for B in AE.CAPS}
    assert got == PLACEMENT
    assert {k: (AE.n_real(k, CUS), AE.grid(k, AE.n_real(k, CUS), CUS), AE.placement(k, AE.n_real(k, CUS), CUS))
            for k in AE.KERNELS} == REAL
    for B in AE.CAPS:
        sz = AE.sizes(B)
        assert max(sz) < 8000 and max(sz) <= AE.N_CAPPED and len(set(sz)) == len(sz)
        assert max(r for r, _ in ROW) >= 6 and sum(p for _, p in ROW) >= 5
    # the maps: every item of the largest size lands in one place, six rounds deep
    for k in AE.KERNELS:
        for B in AE.CAPS:
            n = AE.sizes(B)[-1]
            G = AE.grid(k, n, CUS, B)
            assert G == B
            at = [AE.where(k, i, G) for i in range(n)]
            assert len(set(at)) == n and max(a[2] for a in at) + 1 == AE.rounds(k, n, G) == 6
            assert all(0 <= b < G and 0 <= w < AE.WAVES and 0 <= ln < 64 for b, w, _, ln in at)
            # rounds fill in order: an item's round never falls below an earlier item's
            assert all(at[i][2] <= at[i + 1][2] for i in range(n - 1))


def test_no_word_can_stand_in():
    """All words of the longest bitmap are pairwise distinct and none is 0 or all ones; bits at and past
    n are zero; every one of the 48 MAC bits is flipped by some failing entry of every capped size
    past a round."""
    nmax = max(AE.n_real(k, 304) for k in AE.KERNELS)      # past the MI355X's 256 CUs
    w = AE.mix(np.arange((nmax + 63) // 64))
    assert len(np.unique(w)) == len(w) and not (w == 0).any() and not (w == np.uint64(AE.U64)).any()
    for n in (1, 63, 64, 65, 7889):
        ww = AE.want_words(n)
        assert len(ww) == (n + 63) // 64 and (n % 64 == 0 or int(ww[-1]) >> (n % 64) == 0)
        assert np.array_equal(ww[:-1], w[:len(ww) - 1])
        b = AE.want_bool(n)
        assert len(b) == n and 0 < b.sum() < n or n == 1
    fails = np.nonzero(~AE.want_bool(AE.sizes(1)[-1]))[0]
    assert set((fails % 48).tolist()) == set(range(48))


def _verdicts(mi, exp, kidx, hk, valid):
    """orc_verify_hop_field per entry, the key NULL where the slot is not valid."""
    L = orc.oracle()
    out = np.zeros(len(mi), dtype=bool)
    for i in range(len(mi)):
        s = int(kidx[i]) if kidx is not None else 0
        key = hk[192 * s:192 * s + 192].tobytes() if (int(valid[s >> 5]) >> (s & 31)) & 1 else None
        out[i] = L.orc_verify_hop_field(mi[i].tobytes(), ctypes.c_uint64(int(exp[i])), key)
    return out


def _ref_tags(mi, kidx, hk):
    """The reference's own aes_cmac over the macinputs (oracle/_ref/libaesref.so), or None."""
    R = orc.reference()
    if R is None:
        return None
    out = np.zeros((len(mi), 16), dtype=np.uint8)
    mac = ctypes.create_string_buffer(16)
    for i in range(len(mi)):
        h = hk[192 * int(kidx[i]):192 * int(kidx[i]) + 192].tobytes()
        R.aes_cmac(mi[i].tobytes(), ctypes.c_size_t(16), h[:176], h[176:] + bytes(16), mac)
        out[i] = np.frombuffer(mac.raw, dtype=np.uint8)
    return out


def test_checker_agrees_with_the_designed_bitmap():
    """The capped corpus: orc_verify_hop_field's verdicts are the designed bits, with and without a
    key index; the library's host hfv_verify_macinput and the reference's aes_cmac agree."""
    n = AE.sizes(1)[-1]
    _, hk, valid = AE.full_table()
    for use in (False, True):
        mi, kidx, tags, exp = (a[:n] for a in AE.mac_corpus(AE.N_CAPPED)[use])
        got = _verdicts(mi, exp, kidx if use else None, hk, valid)
        assert np.array_equal(got, AE.want_bool(n))
        assert np.array_equal(AE.pack(got), AE.want_words(n))
        for i in range(0, n, 37):
            s = int(kidx[i]) if use else 0
            assert hfv.verify_macinput(mi[i].tobytes(), int(exp[i]), hk[192 * s:192 * s + 192].tobytes()) == got[i]
            assert orc.cmac(mi[i].tobytes(), AE.full_table()[0][16 * s:16 * s + 16]) == tags[i].tobytes()
        ref = _ref_tags(mi, kidx if use else np.zeros(n, dtype=np.uint8), hk)
        if ref is not None:
            assert np.array_equal(ref, tags)


@pytest.mark.parametrize("name", sorted(AE.EDGE_TABLES))
def test_edge_tables_and_the_five_classes(name):
    valid = AE.EDGE_TABLES[name]
    assert AE.EDGE_TABLES["E"] == {0, 31, 32, 63, 64, 255}
    assert AE.EDGE_TABLES["E"] | AE.EDGE_TABLES["E'"] == set(range(256)) and not AE.EDGE_TABLES["E"] & AE.EDGE_TABLES["E'"]
    assert set(AE.EDGE_SLOTS) == {s for s in range(256) if s % 32 in (0, 1, 30, 31)} | {255}
    # every valid slot of E sits on an end of its validity word, the bit next to it in the word clear
    assert all(s % 32 in (0, 31) for s in AE.E_VALID) and not {1, 30, 33, 62, 65, 254} & AE.EDGE_TABLES["E"]
    mi, ks, exp, cls, want, tags, true = AE.edge_corpus(name)
    _, hk, _ = AE.full_table()
    vw = AE.valid_words(valid)
    assert [int(x) for x in vw] == ([0x80000001, 0x80000001, 1, 0, 0, 0, 0, 0x80000000] if name == "E" else
                                    [0x7ffffffe, 0x7ffffffe, 0xfffffffe, 0xffffffff, 0xffffffff, 0xffffffff,
                                     0xffffffff, 0x7fffffff])
    # every visited slot meets every class, class 3 every bit 48..63
    for s in AE.EDGE_SLOTS:
        mine = ks == s
        assert [int((cls[mine] == c).sum()) for c in range(5)] == [1, 1, 16, 1, 1]
        d = (exp ^ true)[mine]
        assert not (true[mine] >> np.uint64(48)).any() and d[cls[mine] == 0][0] == 0
        assert sorted(int(x) for x in d[cls[mine] == 2]) == [1 << b for b in range(48, 64)]
        flip = int(d[cls[mine] == 1][0])
        assert flip and flip & (flip - 1) == 0 and flip < 1 << 48
        assert int(exp[mine][cls[mine] == 3][0]) == 0
        st = AE.stale_slot(s, valid)
        assert st not in valid and (st == s) == (s not in valid)
    # the checker's own verdicts: only a true MAC in a valid slot passes
    got = _verdicts(mi, exp, ks, hk, vw)
    assert np.array_equal(got, want) and want.sum() == len(set(AE.EDGE_SLOTS) & valid) > 0
    assert np.array_equal(want, (cls == 0) & np.isin(ks, sorted(valid)))
    # ... and were the removed keys still there, class 1 of every slot would pass and nothing else
    # but the stale MACs of removed slots (their own old key)
    full = _verdicts(mi, exp, ks, hk, np.full(8, 0xffffffff, dtype=np.uint32))
    assert np.array_equal(full, (cls == 0) | ((cls == 4) & ~np.isin(ks, sorted(valid))))
    # tags: zero exactly in the removed slots
    assert np.array_equal(~tags.any(axis=1), ~np.isin(ks, sorted(valid)))
    ref = _ref_tags(mi, ks, hk)
    if ref is not None:
        ok = np.isin(ks, sorted(valid))
        assert np.array_equal(ref[ok], tags[ok])


@pytest.mark.parametrize("keysel", [0, 1])
def test_generator_cases_satisfy_the_pass_rule(keysel):
    _, hk, valid = AE.full_table()
    n = AE.sizes(1)[-1]
    firsts = AE.gen_firsts(n)
    assert firsts == (0, 2 ** 30 - 3, 2 ** 32 - 3, 2 ** 62 - 3, 2 ** 64 - n)
    for first in firsts:
        recs = AE.gen_want(n, first, keysel)
        rule = AE.gen_pass_rule(n, first)
        if first + n < 1 << 64:
            assert np.array_equal(rule, orc.expected_pass_rule(n, AE.GEN_SEED, first))
        else:                                           # the last window ends at index 2^64 - 1
            assert np.array_equal(rule[:-1], orc.expected_pass_rule(n - 1, AE.GEN_SEED, first))
        assert np.array_equal(orc.verify_records(recs, hk, valid, keysel), AE.pack(rule))
        assert 0 < (~rule).sum() < n // 8
        # the payload word is the low 32 bits of the index, big-endian
        idx = (first + np.arange(n, dtype=object)) % (1 << 32)
        assert np.array_equal(recs[:, 60:64].astype(np.uint32) @ np.array([1 << 24, 1 << 16, 1 << 8, 1], dtype=np.uint32),
                              np.array(idx.tolist(), dtype=np.uint32))
    # the windows differ from each other (a draw index formed in 32 bits would merge some)
    heads = [AE.gen_want(n, f, keysel)[:8, 40:60].tobytes() for f in firsts + (2 ** 30, 2 ** 32 + 2 ** 30 - 3)]
    assert len(set(heads)) == len(heads)
    assert AE.GEN_STRIDES == (64, 80, 128)


def test_counter_cases():
    recs = AE.count_records(AE.N_CAPPED)
    slots, cons = AE.count_slots(recs), recs[:, 40] & 1
    assert {(int(s), int(c)) for s, c in zip(slots, cons)} == {(s, c) for s in range(256) for c in (0, 1)}
    pre = AE.count_preload()
    assert sorted(np.unique(pre).tolist()) == [0, 2 ** 32 - 3, 2 ** 63] and (pre == 0).sum() > 500
    n = AE.sizes(3)[-1]
    want = AE.count_want(recs, n, pre)
    k = (want - pre)
    assert int(k.sum()) == n and int(k[:, 0].sum()) == int(AE.want_bool(n).sum())
    carry = pre == np.uint64(2 ** 32 - 3)
    assert (k[carry] >= 3).all()                        # every one of them carries out of bit 31
    assert all(int(w) == 2 ** 32 - 3 + int(d) for w, d in zip(want[carry], k[carry]))
    assert np.array_equal(AE.count_slots(recs), np.where(AE.compact(recs)[:, 0] & 1, AE.compact(recs)[:, 11],
                                                         AE.compact(recs)[:, 13]))


def test_expansion_keys_cover_every_carry():
    found = AE.carry_search()
    assert {k: v.hex() for k, v in found.items()} == AE.CARRY_KEYS
    for (p, bit), key in AE.CARRY_KEYS.items():
        assert AE.carries(bytes.fromhex(key))[p] == bit, AE.CARRY_NAMES[p]
    raw, hk = AE.expand_keys()
    assert raw.shape == (257, 16) and hk.shape == (257, 192)
    assert not raw[0].any() and (raw[1] == 255).all()
    assert len({r.tobytes() for r in raw}) >= 257 - 4      # (a key may serve two carry classes)
    # K1 = dbl(L) restated here: shift left by one, xor 0x87 into the last byte where L's msb is set
    for k in range(12):
        L = np.zeros(16, dtype=np.uint8)
        orc.oracle().orc_cypher(orc._vp(np.zeros(16, dtype=np.uint8)), hk[k, :176].tobytes(), orc._vp(L))
        v = int.from_bytes(L.tobytes(), "big")
        k1 = ((v << 1) & ((1 << 128) - 1)) ^ (0x87 if v >> 127 else 0)
        assert hk[k, 176:].tobytes() == k1.to_bytes(16, "big")
        assert hk[k].tobytes() == hfv.hop_key(raw[k].tobytes())


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_hook_only_in_the_test_build():
    assert "hfv_debug_aux_grid" in _exports(hfv.TEST_LIB_PATH)
    assert "hfv_debug_aux_grid" not in _exports(hfv.LIB_PATH)
    assert callable(hfv.Ctx.debug_aux_grid)
