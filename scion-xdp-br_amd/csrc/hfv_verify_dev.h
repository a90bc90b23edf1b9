// hfv_verify_dev.h -- device pieces that more than one hop-field verify kernel uses
// (k_verify_records and k_verify_batches in hfv_verify_kernels.hip, k_verify_service in
// hfv_service_kernel.hip), and the launchers' grid_for.  Only for the .hip units.
#pragma once
#include <hip/hip_runtime.h>

#include "hfv_aes_dev.h"
#include "hfv_internal.h"

namespace hfv {

// ---------------------------------------------------------------------------------------
// record verify: macinput from INF/HF (path_processing.h:39-81), CMAC, 48-bit compare
// ---------------------------------------------------------------------------------------
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

typedef __attribute__((address_space(1))) uint8_t GlobalU8;
typedef __attribute__((address_space(1))) uint64_t GlobalU64;

struct RecWords {
    uint2 inf;    // INF bytes 0-7: flags rsv segid[2] | ts[4]
    uint2 hfa;    // HF bytes 0-7: flags exp ing[2] | eg[2] mac0 mac1
    uint32_t hfb; // HF bytes 8-11: mac2..mac5
};

// One tile's words for the batch-list kernel and the resident service: tile `tile` of the batch
// b (wave-uniform; its recs, n, stride).  The tile's base address is wave-uniform (one SGPR pair)
// and each lane adds a 32-bit offset (global_load ... saddr form); lanes past the batch's last
// record re-read it.  Unconditional loads, so the waitcnt pass can keep a counted vmcnt for a
// prefetch.  NT: non-temporal, for records read once per launch.
template <bool NT, class B>
__device__ __forceinline__ RecWords load_tile(const B &b, uint64_t tile, uint32_t lane, uint32_t inf_off,
                                              uint32_t hf_off)
{
    const uint64_t first = tile * 64;
    const uint64_t left = b.n - 1 - first;                       // uniform: last valid lane
    const uint32_t lim = left < 63 ? (uint32_t)left : 63u;
    const uint32_t off = (lane < lim ? lane : lim) * (uint32_t)b.stride;
    const GlobalU8 *p = (const GlobalU8 *)(b.recs + first * b.stride) + off;
    typedef const __attribute__((address_space(1))) u32x2 *P2;
    typedef const __attribute__((address_space(1))) uint32_t *P1;
    auto ld = [](auto q) { return NT ? __builtin_nontemporal_load(q) : *q; };
    RecWords r;
    const u32x2 x = ld(reinterpret_cast<P2>(p + inf_off));
    const u32x2 y = ld(reinterpret_cast<P2>(p + hf_off));
    r.hfb = ld(reinterpret_cast<P1>(p + hf_off + 8));
    r.inf = make_uint2(x.x, x.y);
    r.hfa = make_uint2(y.x, y.y);
    return r;
}

// macinput words (scion.h:122-132) with the AS-ingress beta rule (path_processing.h:73-77):
// beta = SegID, xor'ed with MAC[0:2] when the Cons flag is clear.
__device__ __forceinline__ void rec_macinput(const RecWords &r, uint32_t w[4])
{
    uint32_t noncons_mask = (r.inf.x & 1u) ? 0u : 0xffff0000u;
    w[0] = (r.inf.x & 0xffff0000u) ^ (r.hfa.y & noncons_mask);
    w[1] = r.inf.y;
    w[2] = r.hfa.x & 0xffffff00u;
    w[3] = r.hfa.y & 0xffffu;
}

// AS-ingress IFID & 0xff (xdp.c:151-157): low byte of the big-endian Cons ? ingress : egress
__device__ __forceinline__ uint32_t rec_key_slot(const RecWords &r)
{
    return (r.inf.x & 1u) ? (r.hfa.x >> 24) : ((r.hfa.y >> 8) & 0xffu);
}

__device__ __forceinline__ bool rec_tag_matches(const RecWords &r, uint32_t t0, uint32_t t1)
{
    uint32_t e0 = __builtin_amdgcn_alignbit(r.hfb, r.hfa.y, 16);   // mac0..mac3
    uint32_t e1 = r.hfb >> 16;                                      // mac4, mac5
    return t0 == e0 && ((t1 ^ e1) & 0xffffu) == 0;
}

// One tile = 64 records = one wave: the verdict ballot (bit L = record L of the tile passed).
// `in`: this lane's record exists.  KEYSEL_ZERO: the wave-uniform slot-0 key (the caller
// handles an empty slot 0); KEYSEL_IFID: the slot's LDS rows, an empty slot fails closed
// (xdp.c:83-84).
// PIN: the round issue order of round_full (the launch kernel's choice, see there).
template <int KEYSEL, bool PIN = false>
__device__ __forceinline__ uint64_t verify_tile(const RecWords &r, bool in, const Lane &l, const UniformKey *ukey)
{
    uint32_t w[4], t0, t1;
    rec_macinput(r, w);
    bool ok = in;
    if constexpr (KEYSEL == HFV_KEYSEL_ZERO) {
        cmac48_macinput<4, UniformKey, PIN>(w, *ukey, l, t0, t1);
    } else {
        const uint32_t slot = rec_key_slot(r);
        cmac48_sched(w, slot, l, t0, t1);
        ok = ok && slot_valid(slot);
    }
    return __ballot(ok && rec_tag_matches(r, t0, t1));
}

// The block's prologue: the round tables from T0 in the kernel arguments (one memory hop, the
// kernarg segment; round 4: 3.0 us from block entry to the fill barrier, against 4.1-4.5 us
// with a second hop to a table image), and config 3's key rows.  nthr: the threads taking part
// (kBlock at every call in hfv_verify_kernels.hip, so that unit's fills are compiled for the
// constant; the service's block 0 fills with one wave fewer).
template <int KEYSEL, class P>
__device__ __forceinline__ void fill_block(P t0, const DevKeyTable *tab, uint32_t nthr)
{
    if (threadIdx.x < nthr) fill_ttab_karg<4>(t0, threadIdx.x >> 6, nthr >> 6);
    if constexpr (KEYSEL == HFV_KEYSEL_IFID) {
        if (threadIdx.x < nthr) fill_keys5(tab, nthr);
    }
}

// The verify kernels' block: 1024 threads, one block per CU.
constexpr int kBlock = 1024;
constexpr uint32_t kWaves = kBlock / 64;

// fill_block's second half for a whole block of kBlock threads whose T0 words are already
// requested (ttab_karg_load<4>(t0, wave, kWaves, f)): the LDS writes, and config 3's key rows.
template <int KEYSEL>
__device__ __forceinline__ void fill_block_store(const TtabFill<4> &f, const DevKeyTable *tab)
{
    ttab_karg_store<4>(threadIdx.x >> 6, kWaves, f);
    if constexpr (KEYSEL == HFV_KEYSEL_IFID) fill_keys5(tab, kBlock);
}

// host: blocks for n records in tiles of 64, one wave per tile, at most per_cu blocks per CU
static inline unsigned grid_for(uint64_t n, int block, int num_cus, int per_cu)
{
    uint64_t tiles = (n + 63) / 64;
    uint64_t blocks = (tiles + block / 64 - 1) / (block / 64);
    uint64_t cap = (uint64_t)num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks ? blocks : 1);
}

}  // namespace hfv
