"""The tile dealing of k_br_process (csrc/hfv_br_kernel.hip) and launch_br_process restated in plain
Python, the sizes that stress it, and a corpus of frames on which no dealing error can pass.

TEST INFRASTRUCTURE ONLY.

The model.  A call of n frames is one launch, or, where it counts verdicts and n passes the split cap
(the 32-bit block counters' automatic one, or the test build's hfv_debug_br_split), one launch per piece
of `cap` frames, each dealt on its own.  A launch of T = ceil(n / 64) tiles runs G = min(max(T, 1), CUs)
blocks of 16 waves, or the test build's hfv_debug_br_grid if that is smaller.

  staged    (slot % 16 == 0, slot >= 128, frames 16-byte aligned) block b owns tiles [T*b/G, T*(b+1)/G).
            Its 16 waves each draw a number from the block's counter before the loop and one more after
            every tile; number g is tile T*b/G + g, and a wave ends at the first draw past the range.
            So a block draws its tiles + 16 numbers.  Which wave draws which number is decided at run
            time; staged_deal() plays the draws round-robin, one legal order.
  direct    (every other slot or alignment) wave w of block b runs tiles w*G + b, + 16 G, + 32 G, ...
  detached  (a pinned table marked detached; either kernel) the same static deal, over a loop that
            only stores action 2, verdict 0, egress -1.

owners() counts how often each tile of each piece is run: 1 everywhere.

The sizes.  EDGE_SIZES puts n on and beside a tile edge and on one whole round of one block (1024).
deal_size(B) = 64 * 16 * B * 5 + 37 gives every wave of B blocks five tiles on average, ragged block
ranges for B = 2 and 3, and a last tile of 37 frames.  real_size(CUs) = 64 * (16 * CUs + 300) + 37 has
more tiles than the real grid has waves: the staged blocks own 17 or 18 tiles, so some waves draw a
second tile and some do not, and the direct loop runs a second round for 301 of its waves.

The corpus.  Frame i = 64 t + j is a function of (t, j) alone, so a corpus of n frames is the first n
of any longer one.  Its kind, one of KINDS, comes from the base-5 digits of t: lanes 8 g .. 8 g + 7 hold
kind (digit g of t + lane) % 5, g = 0..5, so two tiles differ in eight lanes for every digit they differ
in, and every eight lanes hold every kind.  Lanes 48..61 hold a fixed pattern with all four odd ingress
ifindices; lanes 62 and 63 hold not-SCION frames on ifindices nothing else uses, whose lengths are
60 + t % 190 and 60 + t / 190 % 190: the byte counters a tile adds name the tile.  The frames are the hop
inputs of BR 1 (br_fuzz.hop_inputs, IPv4) that the router forwards after checking a hop field; lengths
vary by (t, j) and the rest of each 256-byte slot carries a pattern of i.  Every expectation comes from
the CPU checker (tests/orc.py), never from the library."""
import functools

import numpy as np

import br_shift as S
import br_topo as T
import orc
import scion_hfv as hfv

TILE = 64
WAVES = 16                        # kBrStageWaves, and the 1024 / 64 waves of a direct block
WIN = 128                         # kBrWin: the least slot of the staged kernel
SLOT = 256
DIRECT_SLOT = 264                 # slot % 16 != 0
EDGE_SIZES = (1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)
CAPS = (1, 2, 3)
SPLIT = 1000
VARIANTS = ("staged", "direct", "detached")
FORMS = ("staged", "slot264", "offset8")          # the staged kernel and the two ways into the direct one

V = hfv.VERDICT
KINDS = ("forward", "bad_mac", "truncated", "not_scion", "ifindex")
KIND_VERDICT = (V["SCION_FORWARD"], V["INVALID_HF"], V["PARSE_ERROR"], V["NOT_SCION"], V["NO_INTERFACE"])
ODD_IFINDEX = (63, 64, 2, 200)    # the last with counters and a direct table entry, the first without, two unknown
CARRIER_IFINDEX = (40, 41)        # the ingress interfaces of lanes 62 and 63 alone
CARRIER_BASE, CARRIER_MOD = 60, 190
FIXED_KINDS = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 3, 3)   # lanes 48..63
FIXED_ODD = {58: 0, 59: 1, 60: 2, 61: 3}                          # lane -> ODD_IFINDEX of the fixed ifindex lanes
FILL_ACTION = FILL_VERDICT = 0x5A  # no xdp action (0..4) and no verdict (0, 12, 17, ..., 81)
FILL_EGRESS = -77                  # no ifindex, and not -1
HK = orc.hop_key(T.KEYS[1])


# ---- the model ----------------------------------------------------------------------------------

def deal_size(blocks):
    return TILE * WAVES * blocks * 5 + 37


def real_size(cus):
    return TILE * (WAVES * cus + 300) + 37


def tiles(n):
    return (n + TILE - 1) // TILE


def grid(n, cus, cap=0):
    """Blocks of one launch of n frames: one per tile up to one per CU, and the test cap if smaller."""
    g = min(max(tiles(n), 1), cus)
    return min(g, cap) if cap else g


def split_cap(cus, split=0, maxlen=SLOT):
    """Frames per piece of a counting call: no block may count 2^32 bytes (its share plus two tiles
    of rounding, each frame of maxlen bytes), or the test build's smaller hfv_debug_br_split."""
    per_block = 0xFFFFFFFF // max(maxlen, 1)
    cap_n = (per_block - 128 if per_block > 128 else 1) * cus
    return min(cap_n, split) if split else cap_n


def pieces(n, cus, split=0, counted=True, maxlen=SLOT):
    """[(first frame, frames)] of the launches of one call."""
    cap_n = split_cap(cus, split, maxlen)
    if not counted or n <= cap_n:
        return [(0, n)]
    return [(off, min(cap_n, n - off)) for off in range(0, n, cap_n)]


def block_ranges(T_, G):
    return [(T_ * b // G, T_ * (b + 1) // G) for b in range(G)]


def staged_deal(T_, G):
    """Per block (range, draws, tiles per wave): the 16 waves draw in turn, a wave out at its first
    number past the range."""
    out = []
    for tb0, tb1 in block_ranges(T_, G):
        nxt, mine, live = 0, [[] for _ in range(WAVES)], list(range(WAVES))
        while live:
            still = []
            for w in live:
                t, nxt = tb0 + nxt, nxt + 1
                if t < tb1:
                    mine[w].append(t)
                    still.append(w)
            live = still
        out.append(((tb0, tb1), nxt, mine))
    return out


def static_deal(T_, G):
    """{(block, wave): tiles}: start w * G + b, stride 16 * G."""
    return {(b, w): list(range(w * G + b, T_, WAVES * G)) for b in range(G) for w in range(WAVES)}


def owners(n, variant, cus, cap=0, split=0, counted=True):
    """How often each tile of each piece of the call is run, the pieces' tiles one after the other."""
    out = []
    for _, m in pieces(n, cus, split, counted):
        T_, G = tiles(m), grid(m, cus, cap)
        cnt = np.zeros(T_, dtype=np.int64)
        if variant == "staged":
            for _, _, mine in staged_deal(T_, G):
                for ts in mine:
                    np.add.at(cnt, ts, 1)
        else:
            for ts in static_deal(T_, G).values():
                np.add.at(cnt, ts, 1)
        out.append(cnt)
    return np.concatenate(out)


# ---- the corpus ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bases():
    """(rows u8[m, 256], length, ifindex, PathMeta offset, hop field offset, MAC offset): the IPv4 hop
    inputs of BR 1 that the checker forwards and, with a MAC bit flipped, drops as INVALID_HF."""
    cfg = T.br_config("br1")
    mine = [(i, f) for b, i, f in S.hop_inputs(False) if b == "br1"]
    rows, lens = T.to_slots([f for _, f in mine], slot=SLOT)
    ifx = np.array([i for i, _ in mine], np.uint32)
    offs = [S.field_offsets(f) for _, f in mine]
    bad = rows.copy()
    for k, o in enumerate(offs):
        bad[k, o["mac"][0]] ^= 1
    fwd = orc.br_process(rows.copy(), lens, ifx, cfg, HK)[1] == V["SCION_FORWARD"]
    inv = orc.br_process(bad, lens, ifx, cfg, HK)[1] == V["INVALID_HF"]
    keep = np.nonzero(fwd & inv)[0]
    assert len(keep) >= 8
    out = (rows[keep], lens[keep].astype(np.int64), ifx[keep], np.array([offs[k]["meta"][0] for k in keep]),
           np.array([offs[k]["hf_off"] for k in keep]), np.array([offs[k]["mac"][0] for k in keep]))
    for a in out:
        a.setflags(write=False)
    return out


def kinds(n):
    """Index into KINDS of every frame of an n-frame corpus."""
    i = np.arange(n, dtype=np.int64)
    t, j = i // TILE, i % TILE
    digit = (t // 5 ** np.minimum(j // 8, 5)) % 5
    return np.where(j < 48, (digit + j) % 5, np.array(FIXED_KINDS)[np.maximum(j - 48, 0)])


@functools.lru_cache(maxsize=4)
def corpus(n):
    """(frames u8[n, 256], lens u16[n], ifindex u32[n]).  Read-only."""
    rows, nat, ifi, meta, hf, mac = bases()
    i = np.arange(n, dtype=np.int64)
    t, j = i // TILE, i % TILE
    kind = kinds(n)
    b = (7 * t + 3 * j) % len(rows)
    frames = rows[b]
    col = np.arange(SLOT, dtype=np.int64)
    fill = ((37 * i[:, None] + 11 * col[None, :]) & 0xFF | 1).astype(np.uint8)
    frames = np.where(col[None, :] >= nat[b][:, None], fill, frames)
    lens = nat[b] + (t + 5 * j) % 23
    ifidx = ifi[b].astype(np.int64)
    k = np.nonzero(kind == 1)[0]
    frames[k, mac[b[k]] + i[k] % 6] ^= (1 << (i[k] % 8)).astype(np.uint8)
    k = np.nonzero(kind == 2)[0]
    lens[k] = meta[b[k]] + (5 * i[k] + t[k]) % (hf[b[k]] + 12 - meta[b[k]])
    k = np.nonzero(kind == 3)[0]
    frames[k, 12], frames[k, 13] = 0x08, 0x06                     # ARP
    k = np.nonzero(kind == 4)[0]
    ifidx[k] = np.array(ODD_IFINDEX)[np.where(j[k] >= 48, np.array([FIXED_ODD.get(x, 0) for x in range(TILE)])[j[k]],
                                              (t[k] + j[k]) % 4)]
    for lane, ifx, ln in ((62, CARRIER_IFINDEX[0], t % CARRIER_MOD), (63, CARRIER_IFINDEX[1], t // CARRIER_MOD % CARRIER_MOD)):
        k = np.nonzero(j == lane)[0]
        ifidx[k], lens[k] = ifx, CARRIER_BASE + ln[k]
    assert lens.max() <= SLOT and lens.min() > 14
    out = (np.ascontiguousarray(frames), lens.astype(np.uint16), ifidx.astype(np.uint32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def expected(n, hf_check=True):
    """((action, verdict, egress, stats), frames out) of the CPU checker over corpus(n).  Read-only."""
    frames, lens, ifidx = corpus(n)
    out = frames.copy()
    res = orc.br_process(out, lens, ifidx, T.br_config("br1"), HK, hf_check=hf_check)
    for a in res + (out,):
        a.setflags(write=False)
    return res, out


def guard_frames(m, first=0):
    """(frames u8[m, 256], lens, ifindex): forwardable frames for the slots around a call."""
    rows, nat, ifi, _, _, _ = bases()
    b = (first + np.arange(m)) % len(rows)
    return rows[b].copy(), nat[b].astype(np.uint16), ifi[b].copy()


def tile_bytes(lens, ifidx, verdict):
    """i64[tiles, 64 * 11]: the bytes each tile adds to the byte counters, by (ifindex, counter)."""
    n = len(lens)
    ok = ifidx < hfv.BR_STATS_IFINDEX
    out = np.zeros((tiles(n), hfv.BR_STATS_IFINDEX * hfv.BR_COUNTERS), dtype=np.int64)
    i = np.nonzero(ok)[0]
    np.add.at(out, (i // TILE, ifidx[i].astype(np.int64) * hfv.BR_COUNTERS + (verdict[i] >> 3)), lens[i].astype(np.int64))
    return out
