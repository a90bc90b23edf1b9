// hfv_verify_kernels.hip -- gfx950 (MI355X) kernels for SCION hop-field AES-CMAC verification:
// the single-launch record verify and the batch-list verify, with their launchers.  The resident
// service is in hfv_service_kernel.hip, the pieces all three share in hfv_verify_dev.h, the
// macinput, key-expansion, generator, counting and stream-read kernels in hfv_aux_kernels.hip.
//
// Replaces the per-packet BPF call chain verify_hop_field -> aes_cmac_16bytes ->
// aes_cypher (br/src/bpf/xdp.c:77-91, aes/include/aes/aes.h:129-141, aes/src/aes.c:249-293)
// with one lane per packet:
//
//   * The four AES round tables T0..T3 live in LDS (128 KiB), replicated 32x so that lane L
//     always reads copy L%32: byte address (x << 8) | (t&1) << 7 | (L&31) << 2 | (t>>1) << 16
//     holds table t at index x.  ds_read_b32 banks are (addr/4) % 32 over each 32-lane half,
//     so every lookup is bank-conflict free whatever the data (hfv_aes_dev.h).
//   * The LDS byte address of a lookup is built with ONE v_perm_b32: byte 1 <- the state
//     byte, byte 0 <- the lane's copy/table bits, byte 2 <- the T2/T3 bit.
//   * Round keys: a single key (KEYSEL_ZERO, the reference rule xdp.c:82) is wave-uniform
//     and stays in SGPRs; per-interface keys (KEYSEL_IFID, config 3) come from five 16-byte
//     LDS rows per slot, the schedule words of rounds 3..10 precomputed (hfv_aes_dev.h).
//   * Verdicts: one __ballot per wave = 64 pass bits per 64 records.
//   * Persistent grid of one 1024-thread block per CU, so the table fill is paid once per
//     block; the next tile's record bytes are loaded while the current tile computes.
//
// Rejected variants measured in rounds 1-4 (bitsliced and hybrid AES, LDS-DMA and VGPR table
// fills, per-lane key rows gathered from L2, the 48 KiB key image beside two tables, two
// packets per lane, 2 blocks per CU) are documented in DESIGN.md and profiles/ab_index.md;
// their code is in the history (commit c3ddbb7).  Nothing read from the environment selects a
// kernel.
#include <hip/hip_runtime.h>
#include <string.h>

#include <hip/hip_ext.h>

#include "hfv_verify_dev.h"

namespace hfv {

// ---------------------------------------------------------------------------------------
// single-launch record verify (k_verify_records)
// ---------------------------------------------------------------------------------------
// Unconditional loads (no branch around them, so the compiler can keep a counted vmcnt for
// the prefetch): lanes past the end re-read the last record and are masked off later.
// Non-temporal: the records are read once per launch.
// Not load_tile, on purpose: a 64-bit index per lane serves strides and counts past its 32-bit lane offsets.
__device__ __forceinline__ RecWords load_rec(const uint8_t *recs, uint64_t stride, uint64_t i, uint64_t last,
                                             uint32_t inf_off, uint32_t hf_off)
{
    RecWords r;
    // global address space, so these are global_load (vmcnt only), not flat loads that also
    // count in lgkmcnt
    const GlobalU8 *p = (const GlobalU8 *)(recs) + (i < last ? i : last) * stride;
    typedef const __attribute__((address_space(1))) u32x2 *P2;
    typedef const __attribute__((address_space(1))) uint32_t *P1;
    const u32x2 a = __builtin_nontemporal_load(reinterpret_cast<P2>(p + inf_off));
    const u32x2 b = __builtin_nontemporal_load(reinterpret_cast<P2>(p + hf_off));
    r.hfb = __builtin_nontemporal_load(reinterpret_cast<P1>(p + hf_off + 8));
    r.inf = make_uint2(a.x, a.y);
    r.hfa = make_uint2(b.x, b.y);
    return r;
}

// STAMP = 1 is a diagnostic build (hfv_debug_verify_stamped, scripts/stamps.py): lane 0 of
// every wave records s_memrealtime (100 MHz, chip-wide) at entry, after the table fill, after
// each of its first 10 tiles and at exit into stamps[wave * 16 + k], and s_memtime after the
// fill and at exit (slots 12, 13) for the in-kernel clock.  Nothing else reads the stamps.
//
// DYN = 1 (the default): block b owns the contiguous tile range [b*T/G, (b+1)*T/G) and its
// waves pull tiles from an LDS counter, so waves that the LDS arbiter serves less often take
// fewer tiles instead of finishing last (a static deal left the last ~20 % of the kernel with
// few waves active: scripts/stamps.py).  A wave claims its next tile before computing the
// current one, so the next tile's record loads overlap the rounds.
// DYN = 0: grid-stride tiles (wave w takes w, w + W, ...), for records in registered host
// memory, where 256 ranges far apart thrash the GPU's translation of 4 KiB host pages
// (zero-copy 2^20: 1.60 -> 1.27 ms).
template <int KEYSEL, int DYN, int STAMP = 0>
__global__ __launch_bounds__(kBlock) void k_verify_records(const DevKeyTable *__restrict__ tab,
                                                           const uint8_t *__restrict__ recs, uint64_t stride,
                                                           uint64_t n, uint32_t inf_off, uint32_t hf_off,
                                                           uint64_t *__restrict__ bits,
                                                           uint64_t *__restrict__ stamps, const RecArgs ka)
{
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t last = n - 1;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = wave_uniform(threadIdx.x / 64);
    uint64_t *st = STAMP ? stamps + ((uint64_t)blockIdx.x * kWaves + wv) * 16 : nullptr;
    if constexpr (STAMP) {
        if (lane == 0) st[0] = __builtin_amdgcn_s_memrealtime();
    }
    // DYN: this block's tile range; static: the grid-stride walk
    const uint64_t b0 = DYN ? ntiles * blockIdx.x / gridDim.x : 0;
    const uint64_t count = DYN ? ntiles * (blockIdx.x + 1) / gridDim.x - b0 : ntiles;
    const uint64_t stride_t = DYN ? kWaves : (uint64_t)gridDim.x * kWaves;
    uint64_t t = DYN ? wv : (uint64_t)blockIdx.x * kWaves + wv;   // the wave's first tile (static)
    UniformKey ukey(ka.key0, ka.key0_ok);   // from the kernel arguments: no second memory hop
    if (DYN && threadIdx.x == 0) s_next_tile = kWaves;
    // the wave's first records are in flight while its share of the tables is written
    RecWords cur = load_rec(recs, stride, (b0 + t) * 64 + lane, last, inf_off, hf_off);
    fill_block<KEYSEL>(ka.t0, tab, kBlock);
    __syncthreads();
    const Lane l = lane_bases();
    if constexpr (STAMP) {
        if (lane == 0) {
            st[1] = __builtin_amdgcn_s_memrealtime();
            st[12] = __builtin_amdgcn_s_memtime();   // shader clock, for the in-kernel frequency
        }
    }
    if constexpr (KEYSEL == HFV_KEYSEL_ZERO) {
        if (!ukey.ok) {   // no key in slot 0: every packet fails closed (xdp.c:83-84)
            for (uint64_t tt = t; tt < count; tt += stride_t)
                if (lane == 0) bits[b0 + tt] = 0;
            return;
        }
    }
    // Verdict words wait in a per-wave stash (lane j: the wave's j-th tile) and go out as one
    // store per 64 tiles: a store per tile sits in the in-order vmcnt queue, and the loop latch
    // (which waits for the prefetched record words) would wait for its write acknowledgement
    // every tile.
    uint64_t st_word = 0, st_tile = 0;
    uint32_t stashed = 0;
    int nst = 0;
    while (t < count) {
        uint64_t nt;
        if constexpr (DYN) {
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(&s_next_tile, 1u);
            nt = wave_uniform(c);
        } else {
            nt = t + stride_t;
        }
        RecWords nxt = load_rec(recs, stride, (b0 + nt) * 64 + lane, last, inf_off, hf_off);
        const uint64_t ballot = verify_tile<KEYSEL, true>(cur, (b0 + t) * 64 + lane < n, l, &ukey);
        if (lane == stashed) {
            st_word = ballot;
            st_tile = b0 + t;
        }
        if (++stashed == 64) {
            ((GlobalU64 *)bits)[st_tile] = st_word;
            stashed = 0;
        }
        if constexpr (STAMP) {
            if (lane == 0 && nst < 10) st[2 + nst] = __builtin_amdgcn_s_memrealtime();
            ++nst;
        }
        cur = nxt;
        t = nt;
    }
    if (lane < stashed) ((GlobalU64 *)bits)[st_tile] = st_word;
    if constexpr (STAMP) {
        if (lane == 0) {
            st[13] = __builtin_amdgcn_s_memtime();
            st[15] = __builtin_amdgcn_s_memrealtime();
            // placement: HW_REG_HW_ID (hwreg 4, all 32 bits) and HW_REG_XCC_ID (hwreg 20)
            st[14] = (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                     ((uint64_t)__builtin_amdgcn_s_getreg((15 << 11) | 20) << 32);
        }
    }
}

// ---------------------------------------------------------------------------------------
// stream-ordered batch list (hfv_verify_batches): up to kBatchMax batches in ONE launch
// ---------------------------------------------------------------------------------------
// The batches' tiles are numbered one after the other (batch j holds global tiles
// [cum[j], cum[j+1])) and block k verifies the contiguous range [T*k/G, T*(k+1)/G) of that
// space, its waves claiming tiles from an LDS counter as k_verify_records does.  A block's
// range spans one or two batches, so a wave changes batch about once per block range: the
// batch's descriptor sits in SGPRs, read from the kernel arguments (scalar loads) only when a
// claim leaves it: the batch of a wave's first tile is found by binary search over cum[]
// (batch_find), every later one by a forward step from the current batch (batch_map).  Against
// the resident service (k_verify_service) this launch has no relay wave, no completion protocol
// and no system-scope verdict stores (the launch is stream ordered: the kernel's end publishes the
// bitmaps), and it pays the table fill once for all of its batches instead of once per batch as a
// launch per batch does.
typedef const __attribute__((address_space(4))) BatchArgs *BArgs;

struct BatchTile {   // the wave's current batch (wave-uniform)
    uint64_t recs, bits, n, stride;
    uint32_t lo, hi;   // its global tiles [lo, hi)
    uint32_t j;
};

__device__ __forceinline__ void batch_enter(BArgs a, uint32_t j, BatchTile &b)
{
    b.j = j;
    b.recs = a->d[j].recs;
    b.bits = a->d[j].bits;
    b.n = a->d[j].n;
    b.stride = a->d[j].stride;
    b.lo = a->cum[j];
    b.hi = a->cum[j + 1];
}

// global tile g -> its batch (g only grows along a wave's claims; g < a->total)
__device__ __forceinline__ void batch_map(BArgs a, uint32_t g, BatchTile &b)
{
    if (g < b.hi) return;
    uint32_t j = b.j + 1;
    while (g >= a->cum[j + 1]) ++j;
    batch_enter(a, j, b);
}

// global tile g -> the j with cum[j] <= g < cum[j + 1] (g < a->total), by binary search: at most
// log2(kBatchMax) + 1 dependent scalar loads, wherever in the list the tile lies.  cum[] is strictly
// increasing (the host drops empty batches).  For a wave's first tile only: batch_map's forward
// step from batch 0 costs a block whose range starts in batch j as many load round trips as j,
// ahead of its first record loads.
__device__ __forceinline__ uint32_t batch_find(BArgs a, uint32_t nb, uint32_t g)
{
    uint32_t lo = 0, len = nb;   // cum[lo] <= g < cum[lo + len]
    while (len > 1) {
        const uint32_t half = len >> 1;
        if (g >= a->cum[lo + half]) {
            lo += half;
            len -= half;
        } else {
            len = half;
        }
    }
    return lo;
}

// global tile g of batch b (non-temporal: the records are read once per launch)
__device__ __forceinline__ RecWords batch_load(const BatchTile &b, uint32_t g, uint32_t lane, uint32_t inf_off,
                                               uint32_t hf_off)
{
    return load_tile<true>(b, g - b.lo, lane, inf_off, hf_off);
}

// The next tile's record loads are in flight while the current one is verified, as in
// k_verify_records.  Every load is issued unconditionally (a claim past the block's range re-reads
// its last tile), so the waitcnt pass keeps a counted vmcnt for the tile ahead instead of a vmcnt(0).
// HFV_MUT_TILEDEAL=N (make tiledeal; 0: the product): one deliberately wrong step in the tile dealing
// of k_verify_batches, which tests/test_gpu_tile_deal.py must fail on.  Every mutant only masks
// wrongly, or skips a store it owes to a bitmap: none moves a load or a store.
//   1  the flush of 64 stashed verdict words leaves out lane 63's store
//   2  the rec < n mask takes n from the newest mapped batch (the prefetched claim's), not the tile's own
//   3  the fail-closed loop zeroes only each wave's first tile
//   4  the LDS tile counter starts one too high: the block's 17th tile is never claimed
#ifndef HFV_MUT_TILEDEAL
#define HFV_MUT_TILEDEAL 0
#endif
template <int KEYSEL>
__global__ __launch_bounds__(kBlock) void k_verify_batches(const BatchArgs args)
{
    const BArgs a = (BArgs)__builtin_amdgcn_kernarg_segment_ptr();
    (void)args;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = wave_uniform(threadIdx.x / 64);
    const uint32_t total = a->total, nb = a->nb;
    const uint32_t b0 = (uint32_t)((uint64_t)total * blockIdx.x / gridDim.x);
    const uint32_t b1 = (uint32_t)((uint64_t)total * (blockIdx.x + 1) / gridDim.x);
    if (b1 == b0) return;   // (the launcher gives every block at least one tile)
    const uint32_t last = b1 - 1;
    const uint32_t inf_off = a->inf_off, hf_off = a->hf_off;
    // diagnostics, stored before the first record loads are issued (a store issued after them would
    // make the loop's first reuse of its data registers wait for every load ahead of it: vmcnt(0))
    if (threadIdx.x == 0 && a->clk) {
        a->clk[4 + blockIdx.x] = __builtin_amdgcn_s_memrealtime();   // the block's entry
        if (blockIdx.x == 0) {                                         // the shader clock over the grid
            a->clk[0] = __builtin_amdgcn_s_memtime();
            a->clk[1] = __builtin_amdgcn_s_memrealtime();
        }
    }
#if HFV_MUT_TILEDEAL == 4
    if (threadIdx.x == 0) s_next_tile = kWaves + 1;
#else
    if (threadIdx.x == 0) s_next_tile = kWaves;
#endif
    auto at = [&](uint32_t x) { return x < b1 ? x : last; };   // the tile a load reads for claim x
    auto claim = [&]() -> uint32_t {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(&s_next_tile, 1u);
        return b0 + wave_uniform(c);
    };
    // Record buffers: the loop is unrolled twice over two fixed register slots, slot u verified in
    // step u while the loads of the next claim land in the other slot, which step u - 1 just
    // verified -- so no loop-carried register copy (which would wait for the loads it copies, a
    // vmcnt(0) at the latch) stands between a tile's loads and its use.
    constexpr int S = 2;
    RecWords buf[S];
    BatchTile bt[S];
    uint32_t gg[S];
    // The prologue's two memory chains start together: the T0 loads of the table fill are issued
    // first, then the wave's first tile (static) is found in cum[] and its record loads are issued,
    // and only then the fill's LDS writes wait for T0 (a counted vmcnt: the record loads are younger
    // and stay in flight while the tables are written).  The slot-0 key rows are asked for ahead
    // of the search as well: named behind the record loads, the compiler sinks their 48 scalar
    // loads to the first use, behind the barrier, one more serial round trip to the kernel
    // arguments per block.  The fill takes threadIdx.x >> 6 for the wave, as fill_block does: the
    // compiler knows its bound and emits four unconditional T0 loads, where the scalar copy wv
    // gave eight behind scalar branches (one-batch launches 16.4 -> 17.4 us).
    TtabFill<4> t0w;
    ttab_karg_load<4>(a->pro.t0, threadIdx.x >> 6, kWaves, t0w);
    gg[0] = b0 + wv;
    UniformKey ukey(a->pro.key0, a->pro.key0_ok);
    batch_enter(a, batch_find(a, nb, at(gg[0])), bt[0]);
    buf[0] = batch_load(bt[0], at(gg[0]), lane, inf_off, hf_off);
    fill_block_store<KEYSEL>(t0w, a->tab);
    __syncthreads();
    const Lane l = lane_bases();
    // verdict words wait in a per-wave stash (lane k: the wave's k-th tile, with its own bitmap
    // address, since a wave's tiles may belong to two batches) and go out as one scattered store
    uint64_t st_word = 0, st_addr = 0;
    uint32_t stashed = 0;
    // KEYSEL_ZERO with slot 0 empty fails every packet closed (xdp.c:83-84): a loop of its own after
    // the tile loop (a verify skipped inside the tile loop would leave the prefetched loads unconsumed
    // on that path, and a store on a path into the loop's header would make its first register reuse
    // wait for it: either way the waitcnt pass drains every load at the loop top)
    const bool fail_closed = KEYSEL == HFV_KEYSEL_ZERO && !ukey.ok;
    // the exits leave the unrolled body straight to `done` (a flag checked at the loop top would
    // route them through the loop's header, whose waitcnt state would then hold the loads they left
    // in flight: a vmcnt(0) there on every iteration)
    if (gg[0] >= b1 || fail_closed) goto done;
    for (;;) {
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int in_slot = (u + 1) % S;   // the free slot; slot u holds the newest mapped batch
            gg[in_slot] = claim();
            bt[in_slot] = bt[u];
            batch_map(a, at(gg[in_slot]), bt[in_slot]);
            buf[in_slot] = batch_load(bt[in_slot], at(gg[in_slot]), lane, inf_off, hf_off);
            const uint64_t rec = (uint64_t)(gg[u] - bt[u].lo) * 64 + lane;
#if HFV_MUT_TILEDEAL == 2
            const uint64_t n_own = bt[in_slot].n;
#else
            const uint64_t n_own = bt[u].n;
#endif
            const uint64_t ballot = verify_tile<KEYSEL, true>(buf[u], rec < n_own, l, &ukey);
            if (lane == stashed) {
                st_word = ballot;
                st_addr = bt[u].bits + (uint64_t)(gg[u] - bt[u].lo) * 8;
            }
            if (++stashed == 64) {
#if HFV_MUT_TILEDEAL == 1
                if (lane != 63)
#endif
                *(GlobalU64 *)st_addr = st_word;
                stashed = 0;
            }
            if (gg[(u + 1) % S] >= b1) goto done;   // claims only grow: every later slot is past the range too
        }
    }
done:
    if (lane < stashed) *(GlobalU64 *)st_addr = st_word;
    if (fail_closed) {   // the block's verdict words are 0
        for (uint32_t g = b0 + wv; g < b1; g += kWaves) {
            batch_map(a, g, bt[0]);
            if (lane == 0) *(GlobalU64 *)(bt[0].bits + (uint64_t)(g - bt[0].lo) * 8) = 0;
#if HFV_MUT_TILEDEAL == 3
            break;
#endif
        }
    }
    if (lane == 0 && a->clk)   // the block's last wave to leave sets its finish stamp
        __hip_atomic_fetch_max(&a->clk[4 + kBatchStampBlocks + blockIdx.x], __builtin_amdgcn_s_memrealtime(),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a->clk) {
        a->clk[2] = __builtin_amdgcn_s_memtime();
        a->clk[3] = __builtin_amdgcn_s_memrealtime();
    }
}

int launch_verify_batches(const LaunchGeom &g, int keysel, const BatchArgs &args, void *stream, void *ev_start,
                          void *ev_stop)
{
    auto k = keysel == HFV_KEYSEL_IFID ? k_verify_batches<HFV_KEYSEL_IFID> : k_verify_batches<HFV_KEYSEL_ZERO>;
    // one block per CU, but no more blocks than tiles: every block owns at least one tile
    uint64_t blocks = args.total;
    if (blocks > (uint64_t)g.num_cus) blocks = (uint64_t)g.num_cus;
    if (g.batch_grid_cap && g.batch_grid_cap < blocks) blocks = g.batch_grid_cap;   // test build only
    hipExtLaunchKernelGGL(k, dim3((unsigned)(blocks ? blocks : 1)), dim3(kBlock), 0, (hipStream_t)stream,
                          (hipEvent_t)ev_start, (hipEvent_t)ev_stop, 0u, args);
    return (int)hipGetLastError();
}

// The argument prologue of the verify kernels (RecArgs, BatchArgs::pro, SvcArgs::pro): slot 0's
// device key rows and valid bit from the key table as last published (null: no key, so every
// KEYSEL_ZERO record fails), and T0.
KeyPrologue key_prologue(const DevKeyTable *host_keys)
{
    KeyPrologue ka;
    memset(&ka, 0, sizeof ka);
    if (host_keys) {
        for (int r = 0; r < kDevKeyRows; ++r) memcpy(&ka.key0[4 * r], host_keys->rows[r][0], 16);
        ka.key0_ok = host_keys->valid[0] & 1u;
    }
    memcpy(ka.t0, kTables.t0, sizeof ka.t0);
    return ka;
}

int launch_verify_records(const LaunchGeom &g, const DevKeyTable *tab, const DevKeyTable *host_keys, int keysel,
                          const uint8_t *recs,
                          size_t stride, size_t n, uint32_t inf_off, uint32_t hf_off, uint64_t *bits, void *stream,
                          void *ev_start, void *ev_stop, bool interleaved)
{
    // Records in device memory: the batch-list kernel with one batch (the same loop as a burst of
    // batches, hfv_verify_batches; its 32-bit lane offsets and tile numbers bound stride and n).
    if (!interleaved && stride <= ((size_t)1 << 24) && n <= ((size_t)1 << 36)) {
        BatchArgs a;
        memset(&a, 0, sizeof a);
        a.tab = tab;
        a.inf_off = inf_off;
        a.hf_off = hf_off;
        a.nb = 1;
        a.total = (uint32_t)((n + 63) / 64);
        a.cum[0] = 0;
        a.cum[1] = a.total;
        a.d[0] = {(uint64_t)(uintptr_t)recs, (uint64_t)(uintptr_t)bits, (uint64_t)n, (uint64_t)stride};
        a.pro = key_prologue(host_keys);
        return launch_verify_batches(g, keysel, a, stream, ev_start, ev_stop);
    }
    using K = void (*)(const DevKeyTable *, const uint8_t *, uint64_t, uint64_t, uint32_t, uint32_t, uint64_t *,
                       uint64_t *, const RecArgs);
    const bool ifid = keysel == HFV_KEYSEL_IFID;
    K k = interleaved ? (ifid ? k_verify_records<HFV_KEYSEL_IFID, 0> : k_verify_records<HFV_KEYSEL_ZERO, 0>)
                      : (ifid ? k_verify_records<HFV_KEYSEL_IFID, 1> : k_verify_records<HFV_KEYSEL_ZERO, 1>);
    const unsigned grid = grid_for(n, kBlock, g.num_cus, 1);
    hipExtLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, (hipEvent_t)ev_start,
                          (hipEvent_t)ev_stop, 0u, tab, recs, (uint64_t)stride, (uint64_t)n, inf_off, hf_off, bits,
                          (uint64_t *)nullptr, key_prologue(host_keys));
    return (int)hipGetLastError();
}

int launch_verify_stamped(const LaunchGeom &g, const DevKeyTable *tab, const DevKeyTable *host_keys, const uint8_t *recs,
                          size_t n, uint64_t *bits, uint64_t *stamps, void *stream)
{
    const unsigned grid = grid_for(n, kBlock, g.num_cus, 1);
    hipLaunchKernelGGL((k_verify_records<HFV_KEYSEL_ZERO, 1, 1>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, tab,
                       recs, (uint64_t)64, (uint64_t)n, (uint32_t)HFV_REC_INF_OFF, (uint32_t)HFV_REC_HF_OFF, bits,
                       stamps, key_prologue(host_keys));
    return (int)hipGetLastError();
}

}  // namespace hfv
