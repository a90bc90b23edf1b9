// hfv_frames_fused_kernel.hip -- raw Ethernet frames in, verdict bits out, in one launch
// (hfv_verify_frames_fused): the parse of k_extract_records and the hop-field CMAC of the verify
// kernels in one kernel, with no record in between.  k_verify_frames takes one batch;
// k_verify_frames_list (further down; hfv_verify_frames_batches) takes a list of batches and runs
// the same tile body (fused_tile) over all of their tiles; k_verify_frames_win
// (hfv_verify_frames_host) runs it over packed header windows and also says which frames the window
// left undecided.
//
// k_verify_frames has one lane per frame and a 64-frame tile per wave at a time.  Per tile it
// stages the first kFrWin bytes of the tile's frames into the wave's LDS rows exactly as the
// extract kernel does (hfv_frames_kernel.hip: length and ifindex asked for first, 8 unconditional
// 16-byte loads, the pin, 33-dword rows, the zeroed pad dword), runs frame_locate through the same
// windowed reader (hfv_frame_reader.h), builds the macinput from the five words of the current
// InfoField and HopField, computes the CMAC with the two-table rounds of the router kernel
// (TAB = 3: 16 KiB of round tables, which leaves the LDS to the staged rows), compares 48 bits and
// stores the wave's ballot as the tile's whole bitmap word: one plain store, nothing read back, so
// the bitmap needs no initialisation.  The extract kernel's waves issue on an eighth of the cycles
// they live; the CMAC's ~265 VALU and ~146 LDS instructions per tile go into the rest.
//
// Grid: persistent, one block per CU, min(CUs, ceil(tiles / waves per block)) blocks.  Block k owns
// the tiles [T*k/G, T*(k+1)/G) and its waves claim them one by one from an LDS counter (a lane-0
// LDS atomic: see KFLAGS in the Makefile), as k_br_process and k_verify_batches do.  After the
// prologue's one __syncthreads() the waves meet no block barrier: a wave whose claim is past the
// block's range leaves.
//
// LDS per block: KEYSEL_ZERO 16 waves x 64 rows x 132 B + 16 KiB tables = 151 556 B;
// KEYSEL_IFID adds the 20 KiB of per-slot key rows (s_keys5), which fits with 12 waves: 138 276 B.
//
// Direction (hfv_verify_frames_rx's rule): a frame from an internal interface is judged with the
// SegID as it stands (scion_as_egress, path_processing.h:140-142), every other frame by the
// AS-ingress rule (path_processing.h:73-77: SegID ^ MAC[0:2] when Cons = 0).  The three-launch
// path folds MAC[0:2] into the record for the verify kernel to cancel; here the internal-link
// case simply leaves the fold out.
//
// KEYSEL_ZERO takes slot 0's key rows and valid bit from the kernel arguments and reads no device
// table; KEYSEL_IFID reads the published table's rows and schedule words (fill_keys5<3>).
//
// The kernel never writes a frame and reads nothing at or past frames + n * slot, lens + n or
// ifindex + n (a tile's rows past the last frame repeat that frame); it writes bitmap words below
// (n + 63) / 64 and status bytes below n only.  Bits >= n of the last word are 0.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <string.h>

#include "hfv_aes_dev.h"
#include "hfv_frame_parse.h"
#include "hfv_frame_reader.h"
#include "hfv_internal.h"
#include "hfv_wave_sync.h"

// HFV_MUT_FUSED=N (make fusededge; 0: the product): one deliberately wrong step of k_verify_frames
// (1-3, which tests/test_gpu_frames_fused.py must fail on; 1 and 2 sit in the tile body both kernels
// share) or of k_verify_frames_list (4-6, which tests/test_gpu_frames_list.py must fail on).  Every
// one only masks wrongly or starts the tile counter wrongly: none moves a load or a store.
//   1  the internal-link case keeps the MAC fold
//   2  lanes past the last frame of the last tile vote with the clamped frame
//   3  the LDS tile counter starts one too high: each block's first tile is never verified
//   4  a batch that is not the last of its launch votes with all 64 lanes in its last tile: the
//      clamped frame's verdict leaks into bits at or past n
//   5  after a change of batch the wave keeps the previous batch's "ifindex is NULL" decision for
//      the internal flag (the ifindex load itself stays guarded by the real pointer)
//   6  the list kernel's LDS tile counter starts at 1
#ifndef HFV_MUT_FUSED
#define HFV_MUT_FUSED 0
#endif
// HFV_MUT_HOSTWIN=N (make hostwin; 0: the product): one wrong step of hfv_verify_frames_host, which
// tests/test_gpu_frames_hostmem.py must fail on.  1 and 3 sit in the windowed tile body below, 2 in
// the host's second run (hfv_host_path.cpp).  Every one only masks or indexes wrongly.
//   1  a bound stop at the window is reported as final: the frame is never run again
//   2  the second run's verdict lands on the frame's index within the bounce chunk, not its own
//   3  the retry word of a chunk's last, partial tile votes with all 64 lanes
#ifndef HFV_MUT_HOSTWIN
#define HFV_MUT_HOSTWIN 0
#endif

namespace hfv {

constexpr int fused_waves(int keysel) { return keysel == HFV_KEYSEL_IFID ? 12 : 16; }

static __shared__ uint32_t s_fu_next;   // the block's tile queue head

// One 64-frame tile of one batch, by one wave: tile t of batch `a` (its frames, slot, lens, ifindex,
// status and bits; nf frames of the tile exist, rows past the last frame repeat that frame), staged
// into `rows` (WIN > 0) or read from global memory, located, MACed and compared; the ballot of the
// lanes below nvote (= nf) goes out as bits[t] in one store, the status bytes of the lanes below nf
// where status is not null.  all_external: no frame of the batch is internal, whatever ifindex
// holds.  Every argument but lane and l is wave-uniform.  Shared by k_verify_frames (Batch =
// FusedArgs) and k_verify_frames_list (FrameBatchCur).
//
// WINDOWED (k_verify_frames_win): a.frames holds packed header windows, `window` bytes per frame at a
// stride of `window`, and a.slot is still what the lengths are clamped to.  The parse runs with
// min(len, slot, window), so it reads no byte at or past the window; a frame it leaves undecided (a
// bound stop, more of the frame past the window) votes into retry[t], a second ballot word stored
// whole like the verdict word, and its verdict bit is 0 (its status is not kFrameOk).
template <int KEYSEL, int WIN, bool WINDOWED = false, class Batch>
__device__ __forceinline__ void fused_tile(const Batch &a, const RxSet &set, bool all_external, uint64_t t, uint32_t nf,
                                           uint32_t nvote, uint32_t *rows, uint32_t lane, const UniformKey &ukey,
                                           const Lane &l, uint32_t window = 0u, unsigned long long *retry = nullptr)
{
    const uint64_t base = t * 64;
    const auto stride = [&] {   // bytes between the rows of a.frames
        if constexpr (WINDOWED) return (uint64_t)window;
        else return a.slot;
    }();
    // the lane's own frame (lanes past the last frame: that frame again, never counted), its
    // data_end - data = min(len, slot) and its receiving ifindex: asked for ahead of the rows and
    // pinned once the row loads are issued, as in k_extract_records
    const uint64_t i = base + (lane < nf ? lane : nf - 1);
    const uint32_t len = a.lens[i];
    uint32_t end = len < a.slot ? len : (uint32_t)a.slot;
    uint32_t ifx = 0u;
    if (a.ifindex) ifx = a.ifindex[i];
    if constexpr (WIN > 0) {
        const uint32_t fr_of = lane / kFrC, ch = lane % kFrC;
        fr_v4u pre[kFrC];
#pragma unroll
        for (int r = 0; r < kFrC; ++r) {
            uint32_t fr = r * (64 / kFrC) + fr_of;
            if (fr >= nf) fr = nf - 1;
            pre[r] = *reinterpret_cast<const fr_v4u *>(a.frames + (base + fr) * stride + 16u * ch);
        }
        asm volatile("" : "+v"(end), "+v"(ifx));   // no instruction: the length and ifindex loads are complete here
#pragma unroll
        for (int r = 0; r < kFrC; ++r) {
            uint32_t *d = rows + (r * (64 / kFrC) + fr_of) * kFrRow + 4 * ch;
            d[0] = pre[r].x; d[1] = pre[r].y; d[2] = pre[r].z; d[3] = pre[r].w;
        }
        rows[lane * kFrRow + kFrWin / 4] = 0u;   // the lane's pad dword: read (and shifted out) by u32(124)
        wave_sync();
    }
    const FrameReader<WIN> rd = {rows + lane * kFrRow, a.frames + i * stride};
    uint32_t pend = end;   // what the parse may read: the frame, or no more of it than was packed
    if constexpr (WINDOWED) pend = window < end ? window : end;
    const FrameLoc loc = frame_locate(rd, (int)pend);
    uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};   // InfoField bytes 0-7, HopField bytes 0-11
    if (loc.status == kFrameOk) {
        w[0] = rd.u32((int)loc.inf);
        w[1] = rd.u32((int)loc.inf + 4);
        w[2] = rd.u32((int)loc.hf);
        w[3] = rd.u32((int)loc.hf + 4);
        w[4] = rd.u32((int)loc.hf + 8);
    }
    bool internal = false;
#pragma unroll
    for (uint32_t k = 0; k < kRxSetMax; ++k) internal |= (k < set.n) & (ifx == set.v[k]);
    if (HFV_MUT_FUSED == 1 || all_external) internal = false;
    // macinput (scion.h:122-132): beta = SegID, ^ MAC[0:2] for Cons = 0 on the AS-ingress side only
    const uint32_t fold = ((w[0] & 1u) || internal) ? 0u : 0xffff0000u;
    const uint32_t mi[4] = {(w[0] & 0xffff0000u) ^ (w[3] & fold), w[1], w[2] & 0xffffff00u, w[3] & 0xffffu};
    uint32_t t0, t1;
    bool ok = (HFV_MUT_FUSED == 2 || lane < nvote) && loc.status == kFrameOk;
    if constexpr (KEYSEL == HFV_KEYSEL_ZERO) {
        cmac48_macinput<3>(mi, ukey, l, t0, t1);
        ok = ok && ukey.ok;   // no key in slot 0: every frame fails closed (xdp.c:83-84)
    } else {
        // AS-ingress IFID & 0xff (xdp.c:151-157), as rec_key_slot takes it from a record
        const uint32_t kslot = (w[0] & 1u) ? (w[2] >> 24) : ((w[3] >> 8) & 0xffu);
        cmac48_sched<3>(mi, kslot, l, t0, t1);
        ok = ok && slot_valid(kslot);
    }
    const uint32_t e0 = __builtin_amdgcn_alignbit(w[4], w[3], 16), e1 = w[4] >> 16;   // mac0..3, mac4..5
    const unsigned long long m = __ballot(ok && t0 == e0 && ((t1 ^ e1) & 0xffffu) == 0);
    if (lane == 0) a.bits[t] = m;
    if constexpr (WINDOWED) {
        // HFV_MUT_HOSTWIN 1: never undecided; 3: a partial tile's lanes past nf vote with the clamped frame
        const bool again = HFV_MUT_HOSTWIN != 1 && loc.bound != 0u && end > window;
        const unsigned long long ra = __ballot((HFV_MUT_HOSTWIN == 3 || lane < nvote) && again);
        if (lane == 0) retry[t] = ra;
    }
    if (a.status && lane < nf) a.status[i] = (uint8_t)loc.status;
    if constexpr (WIN > 0) wave_sync();   // the rows are free for the wave's next tile
}

template <int KEYSEL, int WIN>
__global__ __launch_bounds__(fused_waves(KEYSEL) * 64) void k_verify_frames(const FusedArgs a)
{
    constexpr int kW = fused_waves(KEYSEL);
    __shared__ uint32_t s_rows[WIN > 0 ? kW * 64 * kFrRow : 1];
    fill_ttab<3>();
    if constexpr (KEYSEL == HFV_KEYSEL_IFID) fill_keys5<3>(a.tab, kW * 64);
    if (threadIdx.x == 0) s_fu_next = HFV_MUT_FUSED == 3 ? 1u : 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint64_t ntiles = (a.n + 63) / 64;
    const uint64_t tb0 = ntiles * blockIdx.x / gridDim.x, tb1 = ntiles * (blockIdx.x + 1) / gridDim.x;
    uint32_t *rows = s_rows + (WIN > 0 ? wib * 64 * kFrRow : 0);
    const UniformKey ukey(a.key0, a.key0_ok);
    const Lane l = lane_bases3();
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(&s_fu_next, 1u);
        const uint64_t t = tb0 + wave_uniform(c);
        if (t >= tb1) break;   // wave-uniform; no block barrier below
        const uint64_t left = a.n - t * 64;
        const uint32_t nf = left < 64 ? (uint32_t)left : 64u;
        fused_tile<KEYSEL, WIN>(a, a.set, false, t, nf, nf, rows, lane, ukey, l);
    }
}

// Packed header windows (hfv_verify_frames_host's pageable path): k_verify_frames with the rows at a
// stride of a.window bytes and the parse clamped to the window (fused_tile, WINDOWED).  Prologue,
// grid, tile dealing and LDS budgets are k_verify_frames' own.
template <int KEYSEL, int WIN>
__global__ __launch_bounds__(fused_waves(KEYSEL) * 64) void k_verify_frames_win(const FusedWinArgs a)
{
    constexpr int kW = fused_waves(KEYSEL);
    __shared__ uint32_t s_rows[WIN > 0 ? kW * 64 * kFrRow : 1];
    fill_ttab<3>();
    if constexpr (KEYSEL == HFV_KEYSEL_IFID) fill_keys5<3>(a.f.tab, kW * 64);
    if (threadIdx.x == 0) s_fu_next = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint64_t ntiles = (a.f.n + 63) / 64;
    const uint64_t tb0 = ntiles * blockIdx.x / gridDim.x, tb1 = ntiles * (blockIdx.x + 1) / gridDim.x;
    uint32_t *rows = s_rows + (WIN > 0 ? wib * 64 * kFrRow : 0);
    const UniformKey ukey(a.f.key0, a.f.key0_ok);
    const Lane l = lane_bases3();
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(&s_fu_next, 1u);
        const uint64_t t = tb0 + wave_uniform(c);
        if (t >= tb1) break;   // wave-uniform; no block barrier below
        const uint64_t left = a.f.n - t * 64;
        const uint32_t nf = left < 64 ? (uint32_t)left : 64u;
        fused_tile<KEYSEL, WIN, true>(a.f, a.f.set, false, t, nf, nf, rows, lane, ukey, l, a.window, a.retry);
    }
}

// ---------------------------------------------------------------------------------------
// a list of frame batches in ONE launch (hfv_verify_frames_batches)
// ---------------------------------------------------------------------------------------
// The batches' tiles are numbered one after the other (batch j holds global tiles
// [cum[j], cum[j+1])) and block k owns the contiguous range [T*k/G, T*(k+1)/G) of that space, its
// waves claiming tiles from the LDS counter as in k_verify_frames.  The wave keeps its current
// batch's descriptor wave-uniform in SGPRs, read from the kernel arguments by scalar loads only
// when a claim leaves the batch, as k_verify_batches does (hfv_verify_kernels.hip): the batch of a
// wave's first tile is found by binary search over cum[], every later one by a forward step, which
// may pass any number of small batches.  A block range may start in the middle of a batch.  Within
// a batch, tile g - cum[j] is verified exactly as k_verify_frames verifies it (fused_tile).  The
// prologue, the LDS budgets and the waves per block are those of k_verify_frames: the table fill,
// the grid's ramp and its tail are paid once for the whole list.
typedef const __attribute__((address_space(4))) FusedListArgs *FLArgs;

struct FrameBatchCur {   // the wave's current batch (wave-uniform)
    const uint8_t *frames;
    const uint16_t *lens;
    const uint32_t *ifindex;
    uint8_t *status;
    unsigned long long *bits;
    uint64_t n;
    uint32_t slot;
    uint32_t lo, hi;   // its global tiles [lo, hi)
    uint32_t j;
};

__device__ __forceinline__ void frame_batch_enter(FLArgs a, uint32_t j, FrameBatchCur &b)
{
    b.j = j;
    b.frames = (const uint8_t *)a->d[j].frames;
    b.lens = (const uint16_t *)a->d[j].lens;
    b.ifindex = (const uint32_t *)a->d[j].ifindex;
    b.status = (uint8_t *)a->d[j].status;
    b.bits = (unsigned long long *)a->d[j].bits;
    b.n = a->d[j].n;
    b.slot = a->d[j].slot;
    b.lo = a->cum[j];
    b.hi = a->cum[j + 1];
}

// global tile g -> the j with cum[j] <= g < cum[j + 1] (g < a->total), by binary search; cum[] is
// strictly increasing (the host drops empty batches).  For a wave's first tile.
__device__ __forceinline__ uint32_t frame_batch_find(FLArgs a, uint32_t nb, uint32_t g)
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

template <int KEYSEL, int WIN>
__global__ __launch_bounds__(fused_waves(KEYSEL) * 64) void k_verify_frames_list(const FusedListArgs args)
{
    // the descriptors and cum[] are indexed at run time: through the kernarg segment, not the by-value copy
    const FLArgs a = (FLArgs)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int kW = fused_waves(KEYSEL);
    __shared__ uint32_t s_rows[WIN > 0 ? kW * 64 * kFrRow : 1];
    fill_ttab<3>();
    if constexpr (KEYSEL == HFV_KEYSEL_IFID) fill_keys5<3>(args.tab, kW * 64);
    if (threadIdx.x == 0) s_fu_next = HFV_MUT_FUSED == 6 ? 1u : 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t total = args.total, nb = args.nb;
    const uint32_t tb0 = (uint32_t)((uint64_t)total * blockIdx.x / gridDim.x);
    const uint32_t tb1 = (uint32_t)((uint64_t)total * (blockIdx.x + 1) / gridDim.x);
    uint32_t *rows = s_rows + (WIN > 0 ? wib * 64 * kFrRow : 0);
    const UniformKey ukey(args.key0, args.key0_ok);
    const Lane l = lane_bases3();
    auto claim = [&]() -> uint32_t {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(&s_fu_next, 1u);
        return tb0 + wave_uniform(c);
    };
    uint32_t g = claim();
    if (g >= tb1) return;   // wave-uniform; no block barrier below
    FrameBatchCur b;
    frame_batch_enter(a, frame_batch_find(a, nb, g), b);
    bool all_external = b.ifindex == nullptr;
    for (;;) {
        const uint64_t t = g - b.lo;   // the tile within its batch
        const uint64_t left = b.n - t * 64;
        const uint32_t nf = left < 64 ? (uint32_t)left : 64u;
        const uint32_t nvote = (HFV_MUT_FUSED == 4 && b.j + 1 < nb) ? 64u : nf;
        fused_tile<KEYSEL, WIN>(b, args.set, all_external, t, nf, nvote, rows, lane, ukey, l);
        g = claim();
        if (g >= tb1) break;
        if (g >= b.hi) {   // claims only grow: a forward step over as many batches as the claim passed
            uint32_t j = b.j + 1;
            while (g >= a->cum[j + 1]) ++j;
            frame_batch_enter(a, j, b);
            if (HFV_MUT_FUSED != 5) all_external = b.ifindex == nullptr;
        }
    }
}

int launch_verify_frames(const LaunchGeom &g, int keysel, FusedArgs a, const DevKeyTable *host_keys, void *stream,
                         void *ev_start, void *ev_stop)
{
    const KeyPrologue pro = key_prologue(host_keys);
    memcpy(a.key0, pro.key0, sizeof a.key0);
    a.key0_ok = pro.key0_ok;
    if (!a.ifindex || a.set.n == 0) {   // every frame is external
        a.ifindex = nullptr;
        a.set.n = 0;
    }
    // the 16-byte staging loads need what launch_extract needs of the frames
    const bool can_stage = a.slot >= (uint64_t)kFrWin && a.slot % 16 == 0 && ((uintptr_t)a.frames & 15) == 0;
    const bool ifid = keysel == HFV_KEYSEL_IFID;
    using K = void (*)(const FusedArgs);
    const K k = ifid ? (can_stage ? k_verify_frames<HFV_KEYSEL_IFID, kFrWin> : k_verify_frames<HFV_KEYSEL_IFID, 0>)
                     : (can_stage ? k_verify_frames<HFV_KEYSEL_ZERO, kFrWin> : k_verify_frames<HFV_KEYSEL_ZERO, 0>);
    const uint64_t waves = (uint64_t)fused_waves(keysel);
    const uint64_t tiles = (a.n + 63) / 64;
    // one block per CU, but no more blocks than the tiles fill: every block owns at least one tile
    uint64_t blocks = (tiles + waves - 1) / waves;
    if (blocks > (uint64_t)g.num_cus) blocks = (uint64_t)g.num_cus;
    if (g.batch_grid_cap && g.batch_grid_cap < blocks) blocks = g.batch_grid_cap;   // test build only
    hipExtLaunchKernelGGL(k, dim3((unsigned)(blocks ? blocks : 1)), dim3((unsigned)waves * 64), 0, (hipStream_t)stream,
                          (hipEvent_t)ev_start, (hipEvent_t)ev_stop, 0u, a);
    return (int)hipGetLastError();
}

int launch_verify_frames_win(const LaunchGeom &g, int keysel, FusedWinArgs a, const DevKeyTable *host_keys,
                             void *stream)
{
    const KeyPrologue pro = key_prologue(host_keys);
    memcpy(a.f.key0, pro.key0, sizeof a.f.key0);
    a.f.key0_ok = pro.key0_ok;
    if (!a.f.ifindex || a.f.set.n == 0) {   // every frame is external
        a.f.ifindex = nullptr;
        a.f.set.n = 0;
    }
    // the 16-byte staging loads read kFrWin bytes of every packed row
    const bool can_stage = a.window >= (uint32_t)kFrWin && a.window % 16 == 0 && ((uintptr_t)a.f.frames & 15) == 0;
    const bool ifid = keysel == HFV_KEYSEL_IFID;
    using K = void (*)(const FusedWinArgs);
    const K k = ifid ? (can_stage ? k_verify_frames_win<HFV_KEYSEL_IFID, kFrWin> : k_verify_frames_win<HFV_KEYSEL_IFID, 0>)
                     : (can_stage ? k_verify_frames_win<HFV_KEYSEL_ZERO, kFrWin> : k_verify_frames_win<HFV_KEYSEL_ZERO, 0>);
    const uint64_t waves = (uint64_t)fused_waves(keysel);
    const uint64_t tiles = (a.f.n + 63) / 64;
    uint64_t blocks = (tiles + waves - 1) / waves;   // the grid of launch_verify_frames
    if (blocks > (uint64_t)g.num_cus) blocks = (uint64_t)g.num_cus;
    if (g.batch_grid_cap && g.batch_grid_cap < blocks) blocks = g.batch_grid_cap;   // test build only
    hipLaunchKernelGGL(k, dim3((unsigned)(blocks ? blocks : 1)), dim3((unsigned)waves * 64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

bool frames_stageable(const uint8_t *frames, size_t slot)
{
    return slot >= (size_t)kFrWin && slot % 16 == 0 && ((uintptr_t)frames & 15) == 0;
}

int launch_verify_frames_list(const LaunchGeom &g, int keysel, bool staged, const FusedListArgs &a, void *stream,
                              void *ev_start, void *ev_stop)
{
    const bool ifid = keysel == HFV_KEYSEL_IFID;
    using K = void (*)(const FusedListArgs);
    const K k = ifid ? (staged ? k_verify_frames_list<HFV_KEYSEL_IFID, kFrWin> : k_verify_frames_list<HFV_KEYSEL_IFID, 0>)
                     : (staged ? k_verify_frames_list<HFV_KEYSEL_ZERO, kFrWin> : k_verify_frames_list<HFV_KEYSEL_ZERO, 0>);
    const uint64_t waves = (uint64_t)fused_waves(keysel);
    // one block per CU, but no more blocks than the tiles fill: every block owns at least one tile
    uint64_t blocks = ((uint64_t)a.total + waves - 1) / waves;
    if (blocks > (uint64_t)g.num_cus) blocks = (uint64_t)g.num_cus;
    if (g.batch_grid_cap && g.batch_grid_cap < blocks) blocks = g.batch_grid_cap;   // test build only
    hipExtLaunchKernelGGL(k, dim3((unsigned)(blocks ? blocks : 1)), dim3((unsigned)waves * 64), 0, (hipStream_t)stream,
                          (hipEvent_t)ev_start, (hipEvent_t)ev_stop, 0u, a);
    return (int)hipGetLastError();
}

}  // namespace hfv
