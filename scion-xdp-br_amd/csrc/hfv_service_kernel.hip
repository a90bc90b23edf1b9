// hfv_service_kernel.hip -- the resident hop-field verify service for gfx950 (MI355X):
// k_verify_service with its descriptor relay, its launcher, and query_geometry, which takes the
// launch geometry's occupancy check from this kernel.  The tile verify it shares with the launch
// kernels is in hfv_verify_dev.h; the LDS table design is described in hfv_verify_kernels.hip.
#include <hip/hip_runtime.h>

#include <hip/hip_ext.h>

#include "hfv_verify_dev.h"

namespace hfv {

// ---------------------------------------------------------------------------------------
// resident verify service (hfv_service_*): one persistent 1024-thread block per CU verifies
// batch after batch while the round tables (and the key image) stay in LDS
// ---------------------------------------------------------------------------------------
// The host posts batch descriptors into a ring in coherent host memory (SvcShared,
// hfv_internal.h); one wave of block 0 relays them into a device-memory mirror that all
// blocks read (svc_relay).  In every batch, block k owns the contiguous tile range
// [T*k/G, T*(k+1)/G) (T = tiles of the batch, G = grid).  Its waves claim tiles from ONE
// block-local counter that runs on across batches: block tile number g belongs to the batch
// b with base_b <= g < base_b + count_b, base_{b+1} = base_b + count_b (modulo 2^32).  Waves
// roll from one batch into the next without a block barrier, so the tail of batch b
// overlaps the start of batch b + 1, and the table fill is paid once per service instead of
// once per batch.
//
// Descriptor cache: batch b sits in s_svc[b % kSvcRing].  The host posts ticket t = b + 1
// only after ticket t - kSvcRing completed, so when a block loads batch L every batch up to
// L - kSvcRing is verified; an unverified claim g therefore lies in one of the newest
// kSvcRing batches and never in the slot being overwritten.  (Round 4 measured a dynamic tail:
// the last 1-2 batches of a run claimed in chunks from device-scope counters instead of fixed
// shares.  Chunks of 32 tiles: -0.5 % grid time, within noise; chunks of 8 from per-XCD
// counters: +11 %, a claim's round trip is as long as the chunk.  Removed;
// profiles/ab_index.md.)
//
// Completion: verdict words are written through (system-scope stores); a wave counts its
// verified tiles in the slot's LDS counter once those stores are acknowledged (vmcnt(0)),
// and the wave that completes the block's share stores the ticket into dev->done[slot][k]
// (svc_complete, device memory); the relay wave forwards a batch's completion to the host
// once every block has reported it.
// The service kernel's argument struct, read in place in the kernarg segment.
typedef const __attribute__((address_space(4))) SvcArgs *KArgs;

__device__ __forceinline__ SvcDescLite karg_desc(KArgs a, uint32_t i)
{
    SvcDescLite d;
    d.recs = a->inl[i].recs;
    d.bits = a->inl[i].bits;
    d.n = a->inl[i].n;
    d.stride = a->inl[i].stride;
    return d;
}
// svc_cum over the kernel argument's weights
__device__ __forceinline__ uint64_t karg_cum(KArgs a, uint64_t k)
{
    SvcWeights w;
    for (int x = 0; x < 8; ++x) w.w[x] = a->weights.w[x];
    w.w0 = a->weights.w0;
    return svc_cum(w, k);
}

struct alignas(16) SvcSlot {
    uint32_t base, count;   // block tile numbers [base, base + count)
    uint32_t done, stop;    // tiles of the batch this block has verified; 1: exit descriptor
    uint64_t recs, bits, n, stride, tile0;   // the batch, and the first tile of the block's range
    uint64_t pad;
};
static __shared__ SvcSlot s_svc[kSvcRing];
static __shared__ uint32_t s_svc_next, s_svc_loaded, s_svc_lock;
// Generation tag of this service grid (kernel argument, gen << 40): the host ring, the device
// mirror and the completion words carry tag | ticket, so words a previous grid left behind
// never match and nothing has to be cleared between grids.
static __shared__ uint64_t s_svc_tag;
// This block's share bounds (SvcWeights): tiles [T * s_svc_c0 / s_svc_w, T * s_svc_c1 / s_svc_w).
static __shared__ uint64_t s_svc_c0, s_svc_c1, s_svc_w;
__device__ __forceinline__ void svc_share(uint64_t ntiles, uint64_t &t0, uint32_t &count)
{
    t0 = ntiles * s_svc_c0 / s_svc_w;
    count = (uint32_t)(ntiles * s_svc_c1 / s_svc_w - t0);
}

struct SvcTile {   // one claimed tile, wave-uniform
    uint64_t recs, bits, n, stride, tile0, tile;   // tile = tile0 + (g - base)
    uint32_t b, base, count;
};
enum SvcClaim { kSvcFound = 0, kSvcStop = 1, kSvcPending = 2 };

__device__ __forceinline__ uint64_t wave_uniform64(uint64_t x)
{
    return (uint64_t)wave_uniform((uint32_t)x) | ((uint64_t)wave_uniform((uint32_t)(x >> 32)) << 32);
}

// This block's share of batch b is verified (one lane).  The verdict words were written
// through to memory (system-scope stores) and every wave waited for their acknowledgement
// before counting its tiles, so nothing of the batch is left in L2.  The completion word goes
// to device memory (agent scope: written through to the memory side, where the relay wave of
// block 0 reads it); no grid-wide atomic (256 blocks on one counter serialise at the
// memory-side atomic unit: ~40 us per batch at 256 blocks, profiles/r01/service/) and no
// host-memory store whose acknowledgement a compute wave would wait for.
__device__ __attribute__((noinline)) void svc_complete(SvcDev *dev, uint64_t tag, uint32_t b)
{
    dev->blk_fin[blockIdx.x] = __builtin_amdgcn_s_memrealtime();   // read by the host after the grid
    dev->blk_clk1[blockIdx.x] = __builtin_amdgcn_s_memtime();
    __hip_atomic_store(&dev->done[b % kSvcRing][blockIdx.x], tag | ((uint64_t)b + 1), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t memrealtime() { return __builtin_amdgcn_s_memrealtime(); }

// Test hook (hfv_debug_relay_delay): a host round trip `us` microseconds longer.
__device__ __forceinline__ void relay_spin(uint32_t us)
{
    if (!us) return;
    const uint64_t t0 = memrealtime();
    while (memrealtime() - t0 < 100ull * us) __builtin_amdgcn_s_sleep(4);
}

// Descriptor relay and completion forwarder: block 0's last wave, all 64 lanes, for the grid's
// life.  It fetches the descriptors the host posts after the inline ones (batches n_inline,
// n_inline + 1, ...) into the device mirror `dev->mir`, in ticket order, up to 64 per host read:
// lane 0 looks at the next slot's seq; once it is posted, every lane reads the seq of one of
// the next 64 slots, the posted prefix's fields are read, copied (write-through agent-scope
// stores) and their seqs published after the fields are acknowledged.  It also forwards batch
// completions to the host ring (dev->done[slot][0..G) -> host->done[slot]), which the host
// needs only while the grid runs (to reuse ring slots, and for hfv_service_poll/wait).  The
// blocks never wait for this wave unless a batch's descriptor was posted after the grid
// started and has not been fetched yet (kRelayBlockWaits).  It owns the idle timeout: after
// idle_ticks without a new post it publishes a stop descriptor.  It leaves as soon as it has
// published a stop: a grid that exits on its stop has verified everything before it, and the
// host infers those completions from the grid's exit, so the relay never holds the grid open.
__device__ __attribute__((noinline)) void svc_relay(KArgs a, uint32_t lane, uint32_t G)
{
    SvcShared *host = a->host;
    SvcDev *dev = a->dev;
    const uint64_t tag = a->tag;
    const uint32_t n_in = a->n_inline;
    bool stop = n_in && a->inl[n_in - 1].n == kSvcStopN;
    uint32_t b = n_in;                       // next batch to relay
    uint32_t stop_b = stop ? n_in - 1 : ~0u;
    uint32_t f = 0;                          // next batch whose completion is forwarded
    uint64_t reads = 0, rticks = 0, rmax = 0, descs = 0, fwd = 0;
    auto timed_wait = [&]() {                // wait for this wave's host reads; account the trip
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    // one host-memory read at grid start: the PCIe round trip this grid saw (diagnostic)
    uint64_t t0 = memrealtime();
    uint64_t probe_v = __hip_atomic_load(&host->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    timed_wait();
    relay_spin(a->relay_delay_us);   // (the test hook's delay counts as part of the round trip)
    const uint64_t probe = memrealtime() - t0 + (probe_v == 0x5eedull ? 1 : 0);
    uint64_t t_idle = memrealtime();
    while (!stop) {
        bool prog = false;
        // is the next slot posted?
        uint64_t s0 = 0;
        t0 = memrealtime();
        if (lane == 0) s0 = __hip_atomic_load(&host->desc[b % kSvcRing].seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        timed_wait();
        relay_spin(a->relay_delay_us);
        uint64_t rt = memrealtime() - t0;
        ++reads;
        rticks += rt;
        rmax = rt > rmax ? rt : rmax;
        if (wave_uniform64(s0) == (tag | ((uint64_t)b + 1))) {
            // read ahead: the seqs of the next 64 slots, then the fields of the posted prefix
            const uint32_t bi = b + lane;
            const uint64_t want = tag | ((uint64_t)bi + 1);
            SvcDesc *h = &host->desc[bi % kSvcRing];
            t0 = memrealtime();
            const uint64_t seq = __hip_atomic_load(&h->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            timed_wait();
            const uint64_t ready = __ballot(seq == want);
            const uint32_t k = ~ready ? (uint32_t)__builtin_ctzll(~ready) : 64u;   // >= 1: lane 0 saw it
            uint64_t recs = 0, bits = 0, n = 0, stride = 0;
            if (lane < k) {   // fields only after their seq was seen (the wait above)
                typedef uint64_t u64x4 __attribute__((ext_vector_type(4)));
                const u64x4 v = __builtin_nontemporal_load(reinterpret_cast<const u64x4 *>(&h->recs));
                recs = v.x;
                bits = v.y;
                n = v.z;
                stride = v.w;
            }
            timed_wait();
            relay_spin(a->relay_delay_us);
            rt = memrealtime() - t0;
            reads += 2;
            rticks += rt;
            rmax = rt > rmax ? rt : rmax;
            const uint64_t stops = __ballot(lane < k && n == kSvcStopN);
            const uint32_t kk = stops ? (uint32_t)__builtin_ctzll(stops) + 1u : k;
            SvcDesc *m = &dev->mir[bi % kSvcRing];
            if (lane < kk) {   // write-through field stores, acknowledged before the seqs
                __hip_atomic_store(&m->recs, recs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&m->bits, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&m->n, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&m->stride, stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane < kk) {
                __hip_atomic_store(&m->seq, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                dev->relay_clock[bi % kSvcRing] = memrealtime();
            }
            if (stops) {
                stop = true;
                stop_b = b + kk - 1;
            }
            b += kk;
            descs += kk;
            prog = true;
            t_idle = memrealtime();
        } else if (memrealtime() - t_idle > a->idle_ticks) {
            if (lane == 0) {
                SvcDesc *m = &dev->mir[b % kSvcRing];
                __hip_atomic_store(&m->n, kSvcStopN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&m->seq, tag | ((uint64_t)b + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&host->status, kSvcIdleTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            stop = true;
            stop_b = b++;
            prog = true;
        }
        // forward the completions of batches every block has reported (none after the stop:
        // the grid's exit tells the host)
        while (!stop && f < b && f < stop_b) {
            const uint64_t want = tag | ((uint64_t)f + 1);
            bool ok = true;
            for (uint32_t k = lane; k < G; k += 64)
                ok = ok && __hip_atomic_load(&dev->done[f % kSvcRing][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want;
            if (__ballot(!ok)) break;
            if (lane == 0) __hip_atomic_store(&host->done[f % kSvcRing], want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            ++f;
            ++fwd;
            prog = true;
        }
        if (!prog) __builtin_amdgcn_s_sleep(8);
    }
    if (lane == 0) {   // read by the host after the grid
        dev->relay[kRelayProbeTicks] = probe;
        dev->relay[kRelayReads] = reads;
        dev->relay[kRelayReadTicks] = rticks;
        dev->relay[kRelayReadMax] = rmax;
        dev->relay[kRelayDescs] = descs;
        dev->relay[kRelayForwarded] = fwd;
        dev->relay[kRelayInline] = n_in;
    }
}

// Load batch b into its slot (one lane, holding s_svc_lock, s_svc_loaded == b) from the
// device mirror.  blocking: poll until the relay publishes it (bounded by a watchdog: the
// relay itself publishes a stop descriptor after idle_ticks); otherwise one look.  Returns
// false if the descriptor is not there yet.
__device__ __attribute__((noinline)) bool svc_load(KArgs a, uint32_t b, bool blocking)
{
    const uint32_t slot = b % kSvcRing;
    SvcDev *dev = a->dev;
    SvcDesc *d = &dev->mir[slot];
    bool stop = false;
    const uint64_t want = s_svc_tag | ((uint64_t)b + 1);
    if (__hip_atomic_load(&d->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
        if (!blocking) return false;
        __hip_atomic_fetch_add(&dev->area[a->launch & 1].block_waits, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t t0 = memrealtime();
        while (__hip_atomic_load(&d->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
            if (memrealtime() - t0 > 2 * a->idle_ticks + 100000000ull) {
                __hip_atomic_store(&a->host->status, kSvcWatchdog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                stop = true;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // fields only after seq was seen
    // the batch's records were written (by a kernel or a copy into device memory) before the
    // host posted it: drop this CU's stale L1 lines (agent scope, buffer_inv sc1)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (blockIdx.x == 0) dev->load_clock[slot] = memrealtime();
    SvcSlot &s = s_svc[slot];
    const SvcSlot &p = s_svc[(b + kSvcRing - 1) % kSvcRing];
    s.base = b ? p.base + p.count : 0u;
    s.done = 0;
    uint64_t n = 0;
    if (!stop) {
        s.recs = __hip_atomic_load(&d->recs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.bits = __hip_atomic_load(&d->bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n = __hip_atomic_load(&d->n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.stride = __hip_atomic_load(&d->stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stop = n == kSvcStopN;
    }
    s.stop = stop;
    if (stop) {
        s.count = 0;
    } else {
        uint64_t t0;
        uint32_t cnt;
        svc_share((n + 63) / 64, t0, cnt);
        s.n = n;
        s.tile0 = t0;
        s.count = cnt;
        if (s.count == 0) svc_complete(dev, a->tag, b);
    }
    __hip_atomic_store(&s_svc_loaded, b + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    return true;
}

// The batches in the kernel arguments (batches 0 .. n_inline - 1, posted before the launch):
// wave 0 of every block fills their LDS slots before the prologue barrier, lane i batch i,
// the slots' base tile numbers by a prefix sum over the lanes.  Their records were written
// before the grid was launched, so no acquire fence is needed for them.
__device__ __attribute__((noinline)) void svc_load_inline(KArgs a, uint32_t lane)
{
    const uint32_t n_in = a->n_inline;
    const uint64_t c0 = karg_cum(a, blockIdx.x), c1 = karg_cum(a, blockIdx.x + 1);
    const uint64_t w = karg_cum(a, gridDim.x);
    uint32_t cnt = 0;
    uint64_t t0 = 0;
    SvcDescLite d = {0, 0, 0, 0};
    bool stop = false;
    if (lane < n_in) {
        d = karg_desc(a, lane);
        stop = d.n == kSvcStopN;
        if (!stop) {
            const uint64_t nt = (d.n + 63) / 64;
            t0 = nt * c0 / w;
            cnt = (uint32_t)(nt * c1 / w - t0);
        }
    }
    uint32_t incl = cnt;   // inclusive prefix sum of the counts over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
        if ((int)lane >= o) incl += y;
    }
    if (lane < n_in) {
        SvcSlot &s = s_svc[lane];
        s.base = incl - cnt;
        s.count = cnt;
        s.done = 0;
        s.stop = stop;
        s.recs = d.recs;
        s.bits = d.bits;
        s.n = d.n;
        s.stride = d.stride;
        s.tile0 = t0;
        if (!stop && cnt == 0) svc_complete(a->dev, a->tag, lane);
    }
    if (lane == 0) s_svc_loaded = n_in;
}

// The wave has just entered batch b: if batch b + 1 is not loaded yet and nobody is loading,
// take one look for its descriptor now, so the block's waves find it loaded when they reach
// the end of batch b instead of waiting there.
__device__ __forceinline__ void svc_prefetch(KArgs a, uint32_t lane, uint32_t b)
{
    if (lane == 0 && __hip_atomic_load(&s_svc_loaded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == b + 1) {
        uint32_t expect = 0;
        if (__hip_atomic_compare_exchange_strong(&s_svc_lock, &expect, 1u, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP)) {
            if (__hip_atomic_load(&s_svc_loaded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == b + 1)
                (void)svc_load(a, b + 1, false);
            __hip_atomic_store(&s_svc_lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// Map block tile number g to its batch (mb: batch of the wave's previous claim, g only
// grows).  Not blocking: kSvcPending if g lies in a batch the host has not posted yet.
__device__ __forceinline__ SvcClaim svc_map(KArgs a, uint32_t lane, uint32_t g, bool blocking, uint32_t &mb,
                                            const SvcTile &hint, SvcTile &t)
{
    if (g - hint.base < hint.count) {   // same batch as the wave's current tile: no LDS reads
        t = hint;
        t.tile = hint.tile0 + (g - hint.base);
        return kSvcFound;
    }
    uint64_t t_wait = 0;
    for (;;) {
        const uint32_t L =
            wave_uniform(__hip_atomic_load(&s_svc_loaded, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
        // The slots hold batches [L - kSvcRing, L); the oldest one's slot is the one a loader
        // of batch L overwrites, possibly right now, and that batch is verified (the host posts
        // ticket t only after ticket t - kSvcRing completed), so g never lies in it: skip it.
        uint32_t lo = L >= kSvcRing ? L - kSvcRing + 1 : 0u;
        if (mb > lo) lo = mb;
        // the loaded batch holding g, searched forward from the wave's current batch (g only
        // grows, so it is almost always mb or mb + 1; a backward search from the newest
        // loaded batch cost one dependent LDS round trip per batch posted ahead: ~10 per
        // batch change when a run's 20 batches are all inline).  Slot header {base, count,
        // done, stop} in one 16-byte read.
        for (uint32_t b = lo; b < L; ++b) {
            const SvcSlot &s = s_svc[b % kSvcRing];
            const uint4 h = *reinterpret_cast<const uint4 *>(&s);
            const uint32_t base = wave_uniform(h.x);
            if ((int32_t)(g - base) < 0) break;   // before this batch: not loaded (cannot happen)
            if (wave_uniform(h.w)) return kSvcStop;
            const uint32_t count = wave_uniform(h.y);
            if (g - base >= count) continue;      // in a later batch
            t.recs = wave_uniform64(s.recs);
            t.bits = wave_uniform64(s.bits);
            t.n = wave_uniform64(s.n);
            t.stride = wave_uniform64(s.stride);
            t.tile0 = wave_uniform64(s.tile0);
            t.tile = t.tile0 + (g - base);
            t.b = b;
            t.base = base;
            t.count = count;
            mb = b;
            return kSvcFound;
        }
        // load batch L (one loader per block at a time)
        uint32_t r = 0;   // 1: loaded or someone else did, 2: not posted yet
        if (lane == 0) {
            uint32_t expect = 0;
            if (__hip_atomic_compare_exchange_strong(&s_svc_lock, &expect, 1u, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_WORKGROUP)) {
                r = 1;
                if (__hip_atomic_load(&s_svc_loaded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == L &&
                    !svc_load(a, L, blocking))
                    r = 2;
                __hip_atomic_store(&s_svc_lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        r = wave_uniform(r);
        if (r == 2 || (r == 0 && !blocking)) return kSvcPending;
        if (r == 0) {
            // watchdog: the loader is bounded by idle_ticks; never wait much longer here
            const uint64_t now = memrealtime();
            if (!t_wait) t_wait = now;
            if (now - t_wait > 2 * a->idle_ticks + 100000000ull) {
                if (lane == 0)
                    __hip_atomic_store(&a->host->status, kSvcWatchdog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return kSvcStop;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
}

// HFV_MUT_SVCDEAL=N (make svcdeal; 0: the product): one deliberately wrong step in the tile dealing
// of k_verify_service, which tests/test_gpu_svc_deal.py must fail on.  Every mutant only masks
// wrongly, or skips a store it owes to a bitmap: none moves a load or a store, and none changes
// what a wave counts as verified or what a block reports as complete, so every ticket still
// completes and the grid still leaves on its stop.
//   1  the flush of 64 stashed verdict words leaves out lane 63's store
//   2  the rec < n mask takes n from the next mapped batch (nx.n), not the tile's own
//   3  KEYSEL_ZERO with slot 0 empty: a wave's first tile is not failed closed, its word is the
//      rec < n mask alone
//   4  the flush in front of a wait for the host (c == kSvcPending) leaves out the last stashed
//      word (reached where a wave runs out of published descriptors: live submits, or a relayed
//      descriptor, the stop included, that the relay has not published yet)
#ifndef HFV_MUT_SVCDEAL
#define HFV_MUT_SVCDEAL 0
#endif
template <int KEYSEL>
__global__ __launch_bounds__(kBlock) void k_verify_service(const SvcArgs args)
{
    // the fields through the kernarg segment pointer (constant address space): no private copy
    // of the 3.3 KiB argument struct, and helpers take the pointer
    const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    (void)args;
    const uint32_t lane = threadIdx.x & 63;
    SvcDev *dev = a->dev;
    UniformKey ukey(a->pro.key0, a->pro.key0_ok);
    const uint32_t inf_off = a->inf_off, hf_off = a->hf_off;
    if (threadIdx.x == 0) {
        s_svc_next = 0;
        s_svc_lock = 0;
        s_svc_tag = a->tag;
        s_svc_c0 = karg_cum(a, blockIdx.x);
        s_svc_c1 = karg_cum(a, blockIdx.x + 1);
        s_svc_w = karg_cum(a, gridDim.x);
    }
    if (threadIdx.x < 64) svc_load_inline(a, lane);   // the batches posted before the launch
    if (blockIdx.x == 0 && threadIdx.x == 64) dev->area[(a->launch + 1) & 1].block_waits = 0;   // next grid's
    // Block 0's last wave relays later-posted descriptors and forwards completions for the
    // grid's life.  It must not be alive at a barrier the other waves wait at (a wave still
    // running holds the barrier), so it passes the table-fill barrier without filling and
    // starts relaying right after it.
    const uint32_t nthr = blockIdx.x == 0 ? 1024 - 64 : 1024;   // threads filling the tables
    const bool relay = blockIdx.x == 0 && threadIdx.x >= nthr;
    fill_block<KEYSEL>(a->pro.t0, a->tab, nthr);
    __syncthreads();
    if (threadIdx.x == 0) {
        dev->blk_start[blockIdx.x] = memrealtime();
        dev->blk_clk0[blockIdx.x] = __builtin_amdgcn_s_memtime();
    }
    if (relay) {   // no barrier follows: the block's other waves go on without it
        svc_relay(a, lane, gridDim.x);
        return;
    }
    const Lane l = lane_bases();
    // KEYSEL_ZERO with slot 0 empty: every packet fails closed (xdp.c:83-84)
    const bool keyok = KEYSEL != HFV_KEYSEL_ZERO || ukey.ok;
    const UniformKey *ukp = KEYSEL == HFV_KEYSEL_ZERO ? &ukey : nullptr;

    if (blockIdx.x == 0 && threadIdx.x == 0) {   // diagnostics: shader clock over the grid's life
        dev->run_clock[0] = __builtin_amdgcn_s_memtime();
        dev->run_clock[1] = memrealtime();
    }
    uint32_t mb = 0;
    SvcTile none;
    none.base = 0;
    none.count = 0;
    // The loop, per tile: wait for the tile's records (loaded one iteration ahead), claim the
    // next tile (LDS atomic, just in time: claiming one iteration ahead made K = 20 grids 2.1-2.4 %
    // longer, profiles/ab_index.md r03_ahead_ab), store the
    // verdict words of a batch the wave left in the previous
    // iteration (so their write acknowledgement arrives while this tile computes and is
    // covered by the next iteration's wait), map the next tile and issue its loads, compute.
    // (Measured with a phase-counter build on the loop this replaces -- claim at the top, store
    // and a vmcnt(0) drain when leaving a batch: claim/map/load 10 %, store/count drain 9-20 %
    // of a wave's cycles.)
    auto claim = [&]() -> uint32_t {
        uint32_t g = 0;
        if (lane == 0) g = __hip_atomic_fetch_add(&s_svc_next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return g;
    };
    SvcTile cur;
    if (svc_map(a, lane, wave_uniform(claim()), true, mb, none, cur) != kSvcFound) return;
    // Verdict words of cur.b's tiles wait in a per-wave stash (lane j: the j-th word) and go
    // out as ONE scattered write-through store, issued at the top of the iteration after the
    // wave left the batch (or filled the stash).  A store per tile would sit in the wave's
    // in-order vmcnt queue in front of the next tile's record loads.  (Collecting a block's
    // words in LDS and writing 512 B chunks instead was not faster.)
    uint64_t st_word = 0, st_tile = 0, st_bits = 0;
    uint32_t stashed = 0;
    bool flush = false;              // the stash holds words to store at the next top
    uint32_t fl_b = 0, fl_count = 0, fl_k = 0;   // ... and the count they complete (fl_k = 0: none)
    uint32_t dc_b = 0, dc_count = 0, dc_k = 0;   // stored last iteration: count after this wait
    uint32_t pending = 0;            // verified tiles of cur.b not handed to a count yet
#if HFV_MUT_SVCDEAL == 3
    bool first_tile = true;
#elif HFV_MUT_SVCDEAL == 4
    bool before_host_wait = false;
#endif
    auto count = [&](uint32_t b, uint32_t cnt, uint32_t k) {   // stores acknowledged (caller waited)
        if (k && lane == 0) {
            const uint32_t old =
                __hip_atomic_fetch_add(&s_svc[b % kSvcRing].done, k, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (old + k == cnt) svc_complete(dev, a->tag, b);
        }
    };
    auto store_stash = [&]() {
#if HFV_MUT_SVCDEAL == 1
        if (lane < stashed && !(stashed == 64 && lane == 63))
#elif HFV_MUT_SVCDEAL == 4
        if (lane < stashed - (before_host_wait ? 1u : 0u))
#else
        if (lane < stashed)
#endif
            __hip_atomic_store(reinterpret_cast<GlobalU64 *>(st_bits) + st_tile, st_word, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        stashed = 0;
    };
    RecWords rc = load_tile<false>(cur, cur.tile, lane, inf_off, hf_off);
    svc_prefetch(a, lane, cur.b);
    for (;;) {
        // This tile's record words (and every earlier store) are complete.  An explicit wait
        // (a builtin, so the waitcnt pass sees it): without it the pass merges the loop's
        // entry paths and puts a vmcnt(0) AFTER the next tile's loads.
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) expcnt(7) lgkmcnt(15)
        count(dc_b, dc_count, dc_k);           // the stores of the previous iteration are acknowledged
        dc_k = 0;
        if (flush) {                           // the batch left in the previous iteration
            store_stash();
            dc_b = fl_b;
            dc_count = fl_count;
            dc_k = fl_k;
            flush = false;
        }
        const uint32_t g = wave_uniform(claim());
        SvcTile nx;
        SvcClaim c = svc_map(a, lane, g, false, mb, cur, nx);
        if (c != kSvcFound) nx = cur;
        RecWords rn = load_tile<false>(nx, nx.tile, lane, inf_off, hf_off);
        uint64_t ballot = 0;   // KEYSEL_ZERO with slot 0 empty: every packet fails closed
#if HFV_MUT_SVCDEAL == 2
        const uint64_t n_own = nx.n;
#else
        const uint64_t n_own = cur.n;
#endif
        if (keyok) ballot = verify_tile<KEYSEL>(rc, cur.tile * 64 + lane < n_own, l, ukp);
#if HFV_MUT_SVCDEAL == 3
        if (!keyok && first_tile) ballot = __ballot(cur.tile * 64 + lane < n_own);
        first_tile = false;
#endif
        if (lane == stashed) {
            st_word = ballot;
            st_tile = cur.tile;
        }
        st_bits = cur.bits;
        ++stashed;
        ++pending;
        const bool leave = c != kSvcFound || nx.b != cur.b;
        if (leave || stashed == 64) {
            flush = true;
            fl_b = cur.b;
            fl_count = cur.count;
            fl_k = leave ? pending : 0;
            if (leave) pending = 0;
        }
        if (c != kSvcFound) {
            // before waiting for the host (or leaving): store and count everything verified,
            // so a host that waits for those batches before posting the next never waits on us
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            count(dc_b, dc_count, dc_k);
            dc_k = 0;
            if (flush) {
#if HFV_MUT_SVCDEAL == 4
                before_host_wait = c == kSvcPending;
#endif
                store_stash();
#if HFV_MUT_SVCDEAL == 4
                before_host_wait = false;
#endif
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                count(fl_b, fl_count, fl_k);
                flush = false;
            }
            if (c == kSvcPending) {
                c = svc_map(a, lane, g, true, mb, none, nx);
                if (c == kSvcFound) rn = load_tile<false>(nx, nx.tile, lane, inf_off, hf_off);
            }
        }
        if (c == kSvcStop) break;
        if (nx.b != cur.b) svc_prefetch(a, lane, nx.b);
        cur = nx;
        rc = rn;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        dev->run_clock[2] = __builtin_amdgcn_s_memtime();
        dev->run_clock[3] = memrealtime();
    }
}

int launch_verify_service(const LaunchGeom &g, int keysel, const SvcArgs &args, void *stream, void *ev_start,
                          void *ev_stop, unsigned *grid_out)
{
    auto k = keysel == HFV_KEYSEL_IFID ? k_verify_service<HFV_KEYSEL_IFID> : k_verify_service<HFV_KEYSEL_ZERO>;
    unsigned grid = g.svc_blocks > 0 && g.svc_blocks < g.num_cus ? (unsigned)g.svc_blocks : (unsigned)g.num_cus;
    if (grid > kSvcMaxBlocks) grid = kSvcMaxBlocks;
    *grid_out = grid;
    hipExtLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, (hipEvent_t)ev_start,
                          (hipEvent_t)ev_stop, 0u, args);
    return (int)hipGetLastError();
}

int query_geometry(int device, LaunchGeom *g)
{
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return (int)e;
    g->num_cus = prop.multiProcessorCount;
    g->svc_blocks = g->num_cus;
    // one 1024-thread block per CU must fit: the service's LDS (tables, config 3's key rows,
    // descriptor cache) is the largest of the verify kernels'
    int occ = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_verify_service<HFV_KEYSEL_IFID>, kBlock, 0);
    if (e != hipSuccess) return (int)e;
    if (occ < 1) return (int)hipErrorInvalidConfiguration;
    return 0;
}

}  // namespace hfv
