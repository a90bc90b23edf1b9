// hfv_frames_kernel.hip -- from raw Ethernet frames to the fixed-layout records the verify
// kernels take (hfv_extract_records), and the status mask of hfv_verify_frames.
//
// k_extract_records runs the frame parser (hfv_frame_parse.h: parse_underlay / parse_scion /
// parse_scion_path, br/src/bpf/parser.h:45-204) with one lane per frame, a 64-frame tile per wave,
// and copies the frame's current InfoField (8 B) and HopField (12 B) into its record.  The parse
// is a chain of dependent reads at offsets that differ per lane, over frames `slot` bytes apart,
// so the staged kernel first brings the first kFrWin bytes of the tile's 64 frames into LDS with
// coalesced 16-byte loads (8 lanes per frame, 8 frames per load instruction: every load
// instruction asks for whole 128-byte lines, all 8 are in flight at once) and parses out of LDS;
// the row pitch of kFrWin / 4 + 1 dwords keeps the staging writes and the per-lane reads free of
// bank conflicts, as in the router kernel (hfv_br_kernel.hip, s_hdr).  The rare field past the
// window (a hop field deep in a long path) is read from the frame in global memory.  No AES
// tables here: a 256-thread block holds 33 KiB of rows, four blocks (16 waves) share a CU, and
// each wave keeps 8 KiB of loads in flight, which covers the HBM latency.  The grid follows the
// tile count, one tile per wave.
//
// The direct kernel (WIN = 0) reads every field from global memory: for frames that the 16-byte
// loads cannot take (a slot below kFrWin or no multiple of 16, a frame buffer not 16-byte
// aligned); it is also the alternative the staged kernel was measured against (3.1x slower at
// 2 KiB slots, profiles/ab_index.md).
//
// The direction-aware instantiations (RX = true: hfv_extract_records_rx) also read the lane's
// receiving ifindex and take the ctx's internal-interface set by value in the kernel arguments,
// so the membership test is up to 16 compares of the lane's value with scalar registers.  For a
// frame that parsed, came from an internal interface and whose InfoField has Cons = 0 they fold
// the HopField's MAC[0:2] into the record's SegID: one masked XOR of two words the copy already
// holds (w[0], w[3]), no LDS, no further global read.  The ifindex load is asked for right after
// the length load and is complete at the same pin, ahead of the staging's waits.  The RX = false
// instantiations take no such arguments (RxArgs<false> is empty) and compile to what they were.
//
// No kernel writes a frame, reads at or past frames + n * slot (a staged row is the first
// kFrWin <= slot bytes of a frame below n; every other read is bounds-checked by the parser
// against min(len, slot)), or uses a staged byte at or past the frame's length.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "hfv_frame_parse.h"
#include "hfv_frame_reader.h"
#include "hfv_internal.h"
#include "hfv_wave_sync.h"

namespace hfv {

constexpr int kFrWaves = 4;   // waves per block

// What only the direction-aware kernels take: the receiving ifindex of every frame (device
// u32[n], never written) and the internal-interface set.
template <bool RX>
struct RxArgs {};
template <>
struct RxArgs<true> {
    const uint32_t *ifindex;
    RxSet set;
};

template <int WIN, bool RX>
__global__ __launch_bounds__(kFrWaves * 64) void k_extract_records(const uint8_t *__restrict__ frames, uint64_t slot,
                                                                 const uint16_t *__restrict__ lens, uint64_t n,
                                                                 uint8_t *__restrict__ recs, uint64_t stride,
                                                                 uint32_t inf_off, uint32_t hf_off,
                                                                 uint8_t *__restrict__ status, const RxArgs<RX> rx)
{
    __shared__ uint32_t s_rows[WIN > 0 ? kFrWaves * 64 * kFrRow : 1];
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint64_t base = ((uint64_t)blockIdx.x * kFrWaves + wib) * 64;   // the wave's tile
    if (base >= n) return;   // wave-uniform; no block barrier below
    const uint64_t left = n - base;
    const uint32_t nf = left < 64 ? (uint32_t)left : 64u;
    uint32_t *rows = s_rows + (WIN > 0 ? wib * 64 * kFrRow : 0);
    // the lane's own frame, and data_end - data = min(len, slot).  The length is asked for ahead of
    // the rows; left to itself the compiler sinks this load to its first use, behind the staging
    // and its waits (a second, serial round trip), so the value is pinned below once the row loads
    // are issued: memory returns loads in order, and the wait there covers this load alone.
    const uint64_t i = base + (lane < nf ? lane : nf - 1);
    const uint32_t len = lens[i];
    uint32_t end = len < slot ? len : (uint32_t)slot;
    uint32_t ifx = 0u;   // the receiving ifindex: same index as the length (below n), same pin
    if constexpr (RX) ifx = rx.ifindex[i];
    if constexpr (WIN > 0) {
        const uint32_t fr_of = lane / kFrC, ch = lane % kFrC;
        fr_v4u pre[kFrC];
#pragma unroll
        for (int r = 0; r < kFrC; ++r) {
            // unconditional (all 8 loads in flight at once): rows past the batch's last frame get
            // that frame's bytes again and are never parsed
            uint32_t fr = r * (64 / kFrC) + fr_of;
            if (fr >= nf) fr = nf - 1;
            pre[r] = *reinterpret_cast<const fr_v4u *>(frames + (base + fr) * slot + 16u * ch);
        }
        // no instruction: `end` (so the length load) is complete here, and with it the ifindex
        if constexpr (RX) asm volatile("" : "+v"(end), "+v"(ifx));
        else asm volatile("" : "+v"(end));
#pragma unroll
        for (int r = 0; r < kFrC; ++r) {
            uint32_t *d = rows + (r * (64 / kFrC) + fr_of) * kFrRow + 4 * ch;
            d[0] = pre[r].x; d[1] = pre[r].y; d[2] = pre[r].z; d[3] = pre[r].w;
        }
        rows[lane * kFrRow + kFrWin / 4] = 0u;   // the lane's pad dword: read (and shifted out) by u32(124)
        wave_sync();
    }
    if (lane >= nf) return;
    const FrameReader<WIN> rd = {rows + lane * kFrRow, frames + i * slot};
    const FrameLoc loc = frame_locate(rd, (int)end);
    uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};
    if (loc.status == kFrameOk) {
        w[0] = rd.u32((int)loc.inf);
        w[1] = rd.u32((int)loc.inf + 4);
        w[2] = rd.u32((int)loc.hf);
        w[3] = rd.u32((int)loc.hf + 4);
        w[4] = rd.u32((int)loc.hf + 8);
    }
    if constexpr (RX) {
        // scion_as_egress (path_processing.h:140-142) verifies a frame from the internal link with
        // the SegID as it stands; the verify kernels apply the AS-ingress rule (SegID ^ MAC[0:2]
        // for Cons = 0), so MAC[0:2] (HopField bytes 6-7) goes into the record's SegID (InfoField
        // bytes 2-3) here and cancels there.  A failed parse has w = 0 and stays 0.
        bool internal = false;
#pragma unroll
        for (uint32_t k = 0; k < kRxSetMax; ++k) internal |= (k < rx.set.n) & (ifx == rx.set.v[k]);
        if (internal && !(w[0] & 1u)) w[0] ^= w[3] & 0xffff0000u;
    }
    // Records: 8-byte stores.  Where the stride leaves room, the 4 bytes after the hop field are
    // written too (zero): with the compact layout (0, 8, stride 24) a wave's three stores then
    // cover its 1536 contiguous bytes completely, and no line goes out partially written.
    uint8_t *rec = recs + i * stride;
    *reinterpret_cast<fr_v2u *>(rec + inf_off) = fr_v2u{w[0], w[1]};
    *reinterpret_cast<fr_v2u *>(rec + hf_off) = fr_v2u{w[2], w[3]};
    if (stride >= (uint64_t)hf_off + 16) *reinterpret_cast<fr_v2u *>(rec + hf_off + 8) = fr_v2u{w[4], 0u};
    else *reinterpret_cast<uint32_t *>(rec + hf_off + 8) = w[4];
    status[i] = (uint8_t)loc.status;
}

// hfv_verify_frames: clear the pass bit of every frame whose parse failed (its record is all
// zeros, which the verify kernel judged like any other record).  One ballot per wave, one
// read-modify-write of the wave's own bitmap word by lane 0; lanes past n vote 0, which keeps the
// bits >= n of the last word clear.
__global__ __launch_bounds__(256) void k_mask_status(const uint8_t *__restrict__ status, uint64_t n,
                                                     unsigned long long *__restrict__ bits)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = i < n && status[i] == 0;
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && (i & ~(uint64_t)63) < n) bits[i >> 6] &= m;
}

template <bool RX>
static int launch_extract(const uint8_t *frames, size_t slot, const uint16_t *len, size_t n, uint8_t *recs,
                          size_t stride, uint32_t inf_off, uint32_t hf_off, uint8_t *status, const RxArgs<RX> &rx,
                          void *stream, void *ev_start, void *ev_stop)
{
    const bool can_stage = slot >= (size_t)kFrWin && slot % 16 == 0 && ((uintptr_t)frames & 15) == 0;
    using K = void (*)(const uint8_t *, uint64_t, const uint16_t *, uint64_t, uint8_t *, uint64_t, uint32_t, uint32_t,
                       uint8_t *, const RxArgs<RX>);
    const K k = can_stage ? k_extract_records<kFrWin, RX> : k_extract_records<0, RX>;
    const uint64_t tiles = ((uint64_t)n + 63) / 64;
    const unsigned grid = (unsigned)((tiles + kFrWaves - 1) / kFrWaves);
    hipExtLaunchKernelGGL(k, dim3(grid), dim3(kFrWaves * 64), 0, (hipStream_t)stream, (hipEvent_t)ev_start,
                          (hipEvent_t)ev_stop, 0u, frames, (uint64_t)slot, len, (uint64_t)n, recs, (uint64_t)stride,
                          inf_off, hf_off, status, rx);
    return (int)hipGetLastError();
}

int launch_extract_records(const uint8_t *frames, size_t slot, const uint16_t *len, size_t n, uint8_t *recs,
                           size_t stride, uint32_t inf_off, uint32_t hf_off, uint8_t *status, void *stream,
                           void *ev_start, void *ev_stop)
{
    return launch_extract<false>(frames, slot, len, n, recs, stride, inf_off, hf_off, status, RxArgs<false>{}, stream,
                                 ev_start, ev_stop);
}

int launch_extract_records_rx(const uint8_t *frames, size_t slot, const uint16_t *len, const uint32_t *ingress_ifindex,
                              const RxSet &set, size_t n, uint8_t *recs, size_t stride, uint32_t inf_off,
                              uint32_t hf_off, uint8_t *status, void *stream, void *ev_start, void *ev_stop)
{
    // no ifindex array or an empty set: every frame is external, which is the direction-blind kernel
    if (!ingress_ifindex || set.n == 0)
        return launch_extract_records(frames, slot, len, n, recs, stride, inf_off, hf_off, status, stream, ev_start,
                                      ev_stop);
    return launch_extract<true>(frames, slot, len, n, recs, stride, inf_off, hf_off, status,
                                RxArgs<true>{ingress_ifindex, set}, stream, ev_start, ev_stop);
}

int launch_mask_status(const uint8_t *status, size_t n, uint64_t *bits, void *stream)
{
    const unsigned grid = (unsigned)(((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(k_mask_status, dim3(grid), dim3(256), 0, (hipStream_t)stream, status, (uint64_t)n,
                       (unsigned long long *)bits);
    return (int)hipGetLastError();
}

}  // namespace hfv
