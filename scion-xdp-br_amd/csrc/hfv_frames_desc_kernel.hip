// hfv_frames_desc_kernel.hip -- frames addressed by descriptors into one buffer in, verdict bits out,
// in one launch (hfv_verify_frames_desc): k_verify_frames (hfv_frames_fused_kernel.hip) for frames
// that lie where the NIC put them.  Frame i is the desc[i].len bytes at umem + desc[i].addr; the
// descriptor carries the receiving ifindex too (struct hfv_frame_desc, the layout of xdp_desc).
//
// Kept from k_verify_frames: one lane per frame and a 64-frame tile per wave at a time; the
// persistent grid of one block per CU, min(CUs, ceil(tiles / waves per block)) blocks, block k owning
// the tiles [T*k/G, T*(k+1)/G), claimed one by one with a lane-0 LDS atomic (KFLAGS in the Makefile);
// fill_ttab<3> / fill_keys5<3>, 16 waves under KEYSEL_ZERO and 12 under KEYSEL_IFID; frame_locate,
// the macinput, cmac48_macinput<3> / cmac48_sched<3>, the 48-bit compare and one ballot store per
// tile; slot 0's key rows in the kernel arguments.  fused_tile itself is not touched.
//
// New here:
//   Descriptor fetch.  Each lane loads its own 16-byte descriptor with one load (a wave reads 1 KiB
//   contiguous; desc is 8-byte aligned, so the load is declared with that alignment).  Lanes past the
//   last frame repeat the last descriptor and never vote.  Validity (frame_desc_ok, hfv_frame_desc.h)
//   is per lane: an invalid lane asks for no chunk, parses with end = 0 (which reads nothing), votes
//   0 and gets status kFrameBadDesc.  The frame loads of a tile wait for its descriptors, a memory
//   round trip the slot kernel's address arithmetic does not have, so a wave claims one tile ahead
//   and asks for that tile's descriptors before it works on the current one.
//   Staging.  Lane (fr_of, ch) = (lane / 8, lane % 8) loads chunk ch of frame r * 8 + fr_of in round
//   r, as in k_verify_frames, but that frame's base and chunk count belong to lane r * 8 + fr_of: three
//   cross-lane reads (ds_bpermute: no LDS bank is touched) per round.  The chunk is the frame's own
//   bytes [16 ch, 16 ch + 16), loaded with one 16-byte load of alignment 1 from umem + addr + 16 ch:
//   gfx950 under the HSA ABI serves unaligned global loads, so the realignment happens on the way
//   into the row and the rows are those of k_verify_frames -- 33 dwords, frame byte b at row byte b,
//   the same windowed reads, the same LDS budget (16 x 64 x 132 B + 16 KiB = 151 556 B; KEYSEL_IFID
//   12 waves + 20 KiB of key rows: 138 276 B).  No 144-byte span, no shift in the reader.
//   Clamping.  A frame's chunk count is nch = min(8, (umem_bytes - addr) / 16, ceil(len / 16)): a
//   chunk is loaded only where all 16 bytes lie inside the buffer and it holds at least one byte of
//   the frame, so no staging load leaves [umem, umem + umem_bytes) whatever addr and len are.  All
//   eight loads are unconditional, as in k_verify_frames: the lane of a chunk that is not to be read
//   fetches its own descriptor a second time instead, and the row bytes it stores lie at or past the
//   frame's win and are never read.  The lane's reader (DescReader) takes bytes below win = 16 nch from
//   the row and every other byte from umem + addr with byte loads, and the parse is bounded by
//   end = len, as in k_verify_frames: a byte at or past len is never asked for, from the row or from
//   memory, so bytes of the last chunk past len (real memory, inside the buffer) never reach the parse.
//   A 60-byte frame that ends at the buffer's end has nch = 3: bytes 48..59 come by byte loads.
//   WIN = 0: no rows; every byte by byte loads from umem + addr (FrameReader<0>'s way).
//
// LDS accesses.  Row stores: in round r lane (fr_of, ch) stores dwords 4 ch .. 4 ch + 3 of row
// r * 8 + fr_of with four ds_write_b32 (the 132-byte pitch leaves no row but every fourth 16-byte
// aligned); dword j of all lanes goes to banks (33 fr_of + 4 ch + j) mod 64, where rows fr_of and
// fr_of + 4 meet (33 * 4 = 132 = 4 mod 64, i.e. one chunk on): two-way conflicts on 7 of 8 chunks,
// exactly k_verify_frames' store pattern, 32 stores per tile beside the CMAC's ~146 LDS
// instructions.  Row reads: lane L reads dword a of row L at bank (33 L + a) mod 64; 33 is odd, so
// for one a the 64 lanes hit 64 different banks -- conflict-free while the lanes' headers have the
// same layout (one IP family, equal path shapes), conflicting only where lanes read different
// offsets in one instruction.  The pad dword (row dword 32) is zeroed per tile: u32 at offset 124
// reads it and shifts it out.
//
// The kernel never writes umem or desc, reads no descriptor at or past desc + n, writes bitmap words
// below (n + 63) / 64 and status bytes below n only; bits >= n of the last word are 0.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <string.h>

#include "hfv_aes_dev.h"
#include "hfv_frame_desc.h"
#include "hfv_frame_parse.h"
#include "hfv_frame_reader.h"
#include "hfv_internal.h"
#include "hfv_wave_sync.h"

// HFV_MUT_DESC=N (make descedge; 0: the product): one deliberately wrong step of k_verify_frames_desc,
// which tests/test_gpu_frames_desc.py must fail on.  Every one only masks or indexes wrongly; on that
// module's inputs (4 KiB guard regions around the buffer) none moves a load or a store outside the
// test's allocation.
//   1  the validity check forgets len and tests only addr < umem_bytes
//   2  the row shift addr & 15 is dropped for the staging rounds r > 0 (the chunk is loaded from the
//      16-byte boundary below it)
//   3  the base and chunk count of frame r * 8 + fr_of are the lane's own, not the owning lane's
//   4  the parse end is not clamped to len: it runs to the end of the staged window (and the window
//      is staged whatever len is)
//   5  lanes past the last frame vote with the repeated descriptor
//   6  an invalid descriptor's status is written, but its frame is still followed and its bit left to
//      the CMAC
#ifndef HFV_MUT_DESC
#define HFV_MUT_DESC 0
#endif

namespace hfv {

constexpr int desc_waves(int keysel) { return keysel == HFV_KEYSEL_IFID ? 12 : 16; }

static __shared__ uint32_t s_dx_next;   // the block's tile queue head

typedef uint32_t dx_desc4 __attribute__((ext_vector_type(4), aligned(8)));    // one descriptor
typedef uint32_t dx_chunk4 __attribute__((ext_vector_type(4), aligned(1)));   // 16 frame bytes, anywhere

// FrameReader (hfv_frame_reader.h) with a lane's own window: bytes below `win` (a multiple of 16, at
// most WIN) from the lane's LDS row, every other byte from the frame in memory.
template <int WIN>
struct DescReader {
    const uint32_t *row;
    const uint8_t *p;
    int win;
    __device__ __forceinline__ uint32_t g8(int off) const { return p[off]; }
    __device__ __forceinline__ uint32_t g16(int off) const { return g8(off) | g8(off + 1) << 8; }
    __device__ __forceinline__ uint32_t u8(int off) const
    {
        if (WIN == 0 || off >= win) return g8(off);
        return reinterpret_cast<const uint8_t *>(row)[off];
    }
    __device__ __forceinline__ uint32_t u16(int off) const   // off even
    {
        if (WIN == 0 || off + 2 > win) return g16(off);
        return *reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(row) + off);
    }
    __device__ __forceinline__ uint32_t u32(int off) const
    {
        if (WIN == 0 || off + 4 > win) return g16(off) | g16(off + 2) << 16;
        const int a = off >> 2;   // row[a + 1] is at most the pad dword, and then shifted out
        const uint64_t two = (uint64_t)row[a + 1] << 32 | row[a];
        return (uint32_t)(two >> (8 * (off & 3)));
    }
};

// The lane's own descriptor of tile t (lanes past the last frame: the last descriptor again, never
// counted): one 16-byte load per lane, 1 KiB contiguous per wave.
__device__ __forceinline__ dx_desc4 desc_fetch(const DescArgs &a, uint64_t t, uint32_t lane)
{
    const uint64_t left = a.n - t * 64;
    const uint32_t nf = left < 64 ? (uint32_t)left : 64u;
    return *reinterpret_cast<const dx_desc4 *>(a.desc + t * 64 + (lane < nf ? lane : nf - 1));
}

// Tile t by one wave: nf of its 64 frames exist, dv is the lane's descriptor (desc_fetch).  Every
// argument but lane, dv and l is wave-uniform.
template <int KEYSEL, int WIN>
__device__ __forceinline__ void desc_tile(const DescArgs &a, uint64_t t, uint32_t nf, const dx_desc4 dv, uint32_t *rows,
                                          uint32_t lane, const UniformKey &ukey, const Lane &l)
{
    const uint64_t i = t * 64 + (lane < nf ? lane : nf - 1);
    const uint32_t alo = dv.x, ahi = dv.y, len = dv.z, ifx = dv.w;
    const uint64_t addr = (uint64_t)ahi << 32 | alo;
    const bool valid = HFV_MUT_DESC == 1 ? addr < a.umem_bytes : frame_desc_ok(addr, len, a.umem_bytes);
    const bool follow = valid || HFV_MUT_DESC == 6;   // the frame is read at all
    const uint32_t end = follow ? len : 0u;
    int win = 0;
    if constexpr (WIN > 0) {
        // whole chunks inside the buffer that hold a byte of the frame
        uint32_t nch = 0;
        if (follow) {
            const uint64_t whole = valid ? (a.umem_bytes - addr) >> 4 : (uint64_t)kFrC;
            nch = whole < (uint64_t)kFrC ? (uint32_t)whole : (uint32_t)kFrC;
            const uint32_t need = len >= (uint32_t)kFrWin ? (uint32_t)kFrC : (len + 15u) >> 4;
            if (HFV_MUT_DESC != 4 && need < nch) nch = need;
        }
        win = 16 * (int)nch;
        const uint32_t fr_of = lane / kFrC, ch = lane % kFrC;
        // Where each round's chunk comes from, first: the cross-lane reads wait for LDS only, and the
        // eight loads then go out back to back, all unconditional, as k_verify_frames' do (a select on
        // the loaded data put an s_waitcnt vmcnt(0) behind every load; eight conditional loads cost
        // 1100 spilled VGPRs).  A lane whose chunk is not to be read loads its own descriptor again,
        // 16 bytes that are there and in cache; what it stores lies at or past the frame's win and is
        // never read.
        const uint8_t *src[kFrC];
#pragma unroll
        for (int r = 0; r < kFrC; ++r) {
            const int owner = r * (64 / kFrC) + (int)fr_of;   // the lane whose frame this round's row holds
            uint32_t lo = __shfl(alo, owner), hi = __shfl(ahi, owner), nc = __shfl(nch, owner);
            if (HFV_MUT_DESC == 3) {
                lo = alo;
                hi = ahi;
                nc = nch;
            }
            uint64_t off = (uint64_t)hi << 32 | lo;
            if (HFV_MUT_DESC == 2 && r > 0) off &= ~(uint64_t)15;
            src[r] = ch < nc ? a.umem + off + 16u * ch : reinterpret_cast<const uint8_t *>(a.desc + i);
        }
        dx_chunk4 pre[kFrC];
#pragma unroll
        for (int r = 0; r < kFrC; ++r) pre[r] = *reinterpret_cast<const dx_chunk4 *>(src[r]);
#pragma unroll
        for (int r = 0; r < kFrC; ++r) {
            uint32_t *d = rows + (r * (64 / kFrC) + fr_of) * kFrRow + 4 * ch;
            d[0] = pre[r].x; d[1] = pre[r].y; d[2] = pre[r].z; d[3] = pre[r].w;
        }
        rows[lane * kFrRow + kFrWin / 4] = 0u;   // the lane's pad dword: read (and shifted out) by u32(124)
        wave_sync();
    }
    const DescReader<WIN> rd = {rows + lane * kFrRow, a.umem + addr, win};
    uint32_t pend = end;   // what the parse may read: the frame's own bytes
    if (HFV_MUT_DESC == 4 && (uint32_t)win > pend) pend = (uint32_t)win;
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
    for (uint32_t k = 0; k < kRxSetMax; ++k) internal |= (k < a.set.n) & (ifx == a.set.v[k]);
    // macinput (scion.h:122-132): beta = SegID, ^ MAC[0:2] for Cons = 0 on the AS-ingress side only
    const uint32_t fold = ((w[0] & 1u) || internal) ? 0u : 0xffff0000u;
    const uint32_t mi[4] = {(w[0] & 0xffff0000u) ^ (w[3] & fold), w[1], w[2] & 0xffffff00u, w[3] & 0xffffu};
    uint32_t t0, t1;
    bool ok = (HFV_MUT_DESC == 5 || lane < nf) && follow && loc.status == kFrameOk;
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
    if (a.status && lane < nf) a.status[i] = (uint8_t)(valid ? loc.status : kFrameBadDesc);
    if constexpr (WIN > 0) wave_sync();   // the rows are free for the wave's next tile
}

template <int KEYSEL, int WIN>
__global__ __launch_bounds__(desc_waves(KEYSEL) * 64) void k_verify_frames_desc(const DescArgs a)
{
    constexpr int kW = desc_waves(KEYSEL);
    __shared__ uint32_t s_rows[WIN > 0 ? kW * 64 * kFrRow : 1];
    fill_ttab<3>();
    if constexpr (KEYSEL == HFV_KEYSEL_IFID) fill_keys5<3>(a.tab, kW * 64);
    if (threadIdx.x == 0) s_dx_next = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint64_t ntiles = (a.n + 63) / 64;
    const uint64_t tb0 = ntiles * blockIdx.x / gridDim.x, tb1 = ntiles * (blockIdx.x + 1) / gridDim.x;
    uint32_t *rows = s_rows + (WIN > 0 ? wib * 64 * kFrRow : 0);
    const UniformKey ukey(a.key0, a.key0_ok);
    const Lane l = lane_bases3();
    auto claim = [&]() -> uint64_t {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(&s_dx_next, 1u);
        return tb0 + wave_uniform(c);
    };
    // The frame loads of a tile wait for its descriptors, a second memory round trip that the slot
    // kernel's address arithmetic does not have.  So the wave claims a tile ahead and asks for that
    // tile's descriptors before it works on the current one: they arrive beside the current tile's
    // frame loads and under its CMAC.
    uint64_t t = claim();
    if (t >= tb1) return;   // wave-uniform; no block barrier below
    dx_desc4 dv = desc_fetch(a, t, lane);
    for (;;) {
        const uint64_t tn = claim();
        const bool more = tn < tb1;   // wave-uniform
        dx_desc4 dn = dv;
        if (more) dn = desc_fetch(a, tn, lane);
        const uint64_t left = a.n - t * 64;
        const uint32_t nf = left < 64 ? (uint32_t)left : 64u;
        desc_tile<KEYSEL, WIN>(a, t, nf, dv, rows, lane, ukey, l);
        if (!more) break;
        t = tn;
        dv = dn;
    }
}

int launch_verify_frames_desc(const LaunchGeom &g, int keysel, DescArgs a, const DevKeyTable *host_keys, void *stream,
                              void *ev_start, void *ev_stop)
{
    const KeyPrologue pro = key_prologue(host_keys);
    memcpy(a.key0, pro.key0, sizeof a.key0);
    a.key0_ok = pro.key0_ok;
    // the staged kernel for a 16-byte aligned buffer that holds a whole window (then descriptors at
    // multiples of 16 get aligned staging loads); the byte-load kernel otherwise, with the same results
    const bool can_stage = a.umem_bytes >= (uint64_t)kFrWin && ((uintptr_t)a.umem & 15) == 0;
    const bool ifid = keysel == HFV_KEYSEL_IFID;
    using K = void (*)(const DescArgs);
    const K k = ifid ? (can_stage ? k_verify_frames_desc<HFV_KEYSEL_IFID, kFrWin> : k_verify_frames_desc<HFV_KEYSEL_IFID, 0>)
                     : (can_stage ? k_verify_frames_desc<HFV_KEYSEL_ZERO, kFrWin> : k_verify_frames_desc<HFV_KEYSEL_ZERO, 0>);
    const uint64_t waves = (uint64_t)desc_waves(keysel);
    const uint64_t tiles = (a.n + 63) / 64;
    // one block per CU, but no more blocks than the tiles fill: every block owns at least one tile
    uint64_t blocks = (tiles + waves - 1) / waves;
    if (blocks > (uint64_t)g.num_cus) blocks = (uint64_t)g.num_cus;
    if (g.batch_grid_cap && g.batch_grid_cap < blocks) blocks = g.batch_grid_cap;   // test build only
    hipExtLaunchKernelGGL(k, dim3((unsigned)(blocks ? blocks : 1)), dim3((unsigned)waves * 64), 0, (hipStream_t)stream,
                          (hipEvent_t)ev_start, (hipEvent_t)ev_stop, 0u, a);
    return (int)hipGetLastError();
}

}  // namespace hfv
