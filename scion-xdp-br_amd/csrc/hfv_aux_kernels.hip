// hfv_aux_kernels.hip -- gfx950 (MI355X) kernels beside the hop-field verify paths: prepared
// macinputs (verify or full tags), key expansion, the synthetic record generator, the verdict
// counters and the diagnostic streaming read, with their launchers.
//
// HFV_MUT_AUX=N (make auxedge; 0: the product): one deliberately wrong step in one of these kernels,
// which tests/test_gpu_aux_edges.py must fail on.  Every mutant picks a wrong index inside the array the
// right one lies in, or drops a condition: none changes a loop's start, step or bound, and none reads or
// writes outside the arrays the product touches.
//   1  k_macinputs (verify) writes the verdict word of every round after a wave's first to the first
//      round's word index
//   2  k_macinputs (tags) does not zero the tag of an invalid key slot
//   3  k_macinputs (verify) masks `expected` to 48 bits as well: bits 48..63 of it are ignored
//   4  k_count_verdicts takes the pass bit from the word of the thread's first round
//   5  k_gen_records forms the draw index 4 * i in 32 bits
//   6  k_gen_records writes row j at j * 64 instead of j * stride
#ifndef HFV_MUT_AUX
#define HFV_MUT_AUX 0
#endif
#include <hip/hip_runtime.h>

#include <hip/hip_ext.h>

#include "hfv_verify_dev.h"

namespace hfv {

// ---------------------------------------------------------------------------------------
// diagnostic: the HBM streaming-read rate of a list of device buffers (hfv_debug_stream_read),
// the achievable peak a bench run prices its verify kernel against -- the same resident batches,
// read densely (16 B per lane per load, non-temporal), 4 blocks of 1024 threads per CU
// (scripts/ubench/stream_read.hip: 7.05 TB/s on a 1 GiB buffer, round 1)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_stream_read(const StreamArgs args)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    uint32_t acc = 0;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint32_t j = 0; j < args.nb; ++j) {
        const u32x4 *p = (const u32x4 *)args.buf[j];
        const uint64_t n = args.bytes[j] / 16;
        for (uint64_t i = tid; i < n; i += nthr) {
            const u32x4 v = __builtin_nontemporal_load(p + i);
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    if (acc == 0x9e3779b9u) args.sink[0] = acc;   // keeps the loads; never true for the bench's records in practice
}

int launch_stream_read(const LaunchGeom &g, const StreamArgs &args, void *stream, void *ev_start, void *ev_stop)
{
    hipExtLaunchKernelGGL(k_stream_read, dim3(4 * g.num_cus), dim3(1024), 0, (hipStream_t)stream,
                          (hipEvent_t)ev_start, (hipEvent_t)ev_stop, 0u, args);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// prepared macinputs: verify (xdp.c:77-91) or full tags (aes_cmac_16bytes)
// ---------------------------------------------------------------------------------------
template <int MODE, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_macinputs(const DevKeyTable *__restrict__ tab,
                                                     const uint4 *__restrict__ mi, const uint2 *__restrict__ expected,
                                                     const uint8_t *__restrict__ kidx, uint64_t n,
                                                     uint64_t *__restrict__ bits, uint4 *__restrict__ tags)
{
    constexpr uint32_t kBlockWaves = BLOCK / 64;
    const uint64_t ntiles = (n + 63) / 64;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_uniform(blockIdx.x * kBlockWaves + threadIdx.x / 64);
    const uint32_t nwaves = gridDim.x * kBlockWaves;
    fill_ttab<2>();
    fill_keys(tab);
    __syncthreads();
    const Lane l = lane_bases();
    for (uint64_t t = wave; t < ntiles; t += nwaves) {
        uint64_t i = t * 64 + lane;
        bool in = i < n;
        uint4 m = in ? mi[i] : make_uint4(0, 0, 0, 0);
        uint32_t slot = (in && kidx) ? kidx[i] : 0u;
        const LdsKey key(slot);
        uint32_t w[4] = {m.x, m.y, m.z, m.w}, s[4];
        cmac_general<2>(w, key, l, s);
        if constexpr (MODE == kModeTags) {
            uint32_t o[4];
            round_last_full<2>(s, key.row(10), l, o);
#if HFV_MUT_AUX != 2
            if (!key.ok()) o[0] = o[1] = o[2] = o[3] = 0;
#endif
            if (in) tags[i] = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            uint32_t t0, t1;
            round_last_48<2>(s, key.row(10), l, t0, t1);
            uint2 e = in ? expected[i] : make_uint2(0, 0);
            // actual = tag bytes 0..5 as LE u64 (upper 16 bits zero) == expected (xdp.c:89-90)
#if HFV_MUT_AUX == 3
            bool pass = in && key.ok() && t0 == e.x && (t1 & 0xffffu) == (e.y & 0xffffu);
#else
            bool pass = in && key.ok() && t0 == e.x && (t1 & 0xffffu) == e.y;
#endif
            uint64_t ballot = __ballot(pass);
#if HFV_MUT_AUX == 1
            if (lane == 0) bits[t < nwaves ? t : wave] = ballot;
#else
            if (lane == 0) bits[t] = ballot;
#endif
        }
    }
}

// ---------------------------------------------------------------------------------------
// key expansion + CMAC subkey, one key per lane (aes.c:120-137, 298-325; br_loader.cpp:215-218)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sbox_g(uint32_t x) { return (c_t0[x & 0xff] >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t sub_word_g(uint32_t w)
{
    return sbox_g(w) | sbox_g(w >> 8) << 8 | sbox_g(w >> 16) << 16 | sbox_g(w >> 24) << 24;
}
__device__ __forceinline__ uint32_t tg(int row, uint32_t x)
{
    uint32_t t = c_t0[x & 0xff];
    return row ? __builtin_amdgcn_alignbit(t, t, 32 - 8 * row) : t;
}
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

__global__ __launch_bounds__(256) void k_expand_keys(const uint4 *__restrict__ raw, uint64_t n,
                                                     hop_key *__restrict__ out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 k = raw[i];
    uint32_t w[44];
    w[0] = k.x; w[1] = k.y; w[2] = k.z; w[3] = k.w;
    uint32_t rcon = 1;
#pragma unroll
    for (int j = 4; j < 44; j += 4) {
        uint32_t t = sub_word_g(__builtin_amdgcn_alignbit(w[j - 1], w[j - 1], 8)) ^ rcon;   // RotWord = rotr8
        rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u);
        w[j] = w[j - 4] ^ t;
        w[j + 1] = w[j - 3] ^ w[j];
        w[j + 2] = w[j - 2] ^ w[j + 1];
        w[j + 3] = w[j - 1] ^ w[j + 2];
    }
    // L = E_K(0^128); K1 = dbl(L) (RFC 4493 2.3)
    uint32_t s[4] = {w[0], w[1], w[2], w[3]}, nn[4];
    for (int r = 1; r < 10; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            nn[c] = tg(0, s[c]) ^ tg(1, s[(c + 1) & 3] >> 8) ^ tg(2, s[(c + 2) & 3] >> 16) ^ tg(3, s[(c + 3) & 3] >> 24) ^
                    w[4 * r + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = nn[c];
    }
    uint32_t L[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        L[c] = (sbox_g(s[c]) | sbox_g(s[(c + 1) & 3] >> 8) << 8 | sbox_g(s[(c + 2) & 3] >> 16) << 16 |
                sbox_g(s[(c + 3) & 3] >> 24) << 24) ^ w[40 + c];
    // big-endian 128-bit shift: byte 0 is the most significant
    uint32_t q0 = bswap(L[0]), q1 = bswap(L[1]), q2 = bswap(L[2]), q3 = bswap(L[3]);
    uint32_t msb = q0 >> 31;
    q0 = (q0 << 1) | (q1 >> 31);
    q1 = (q1 << 1) | (q2 >> 31);
    q2 = (q2 << 1) | (q3 >> 31);
    q3 = (q3 << 1) ^ (msb ? 0x87u : 0u);
    uint32_t k1[4] = {bswap(q0), bswap(q1), bswap(q2), bswap(q3)};
    uint4 *o = reinterpret_cast<uint4 *>(out + i);
#pragma unroll
    for (int r = 0; r < 11; ++r) o[r] = make_uint4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
    o[11] = make_uint4(k1[0], k1[1], k1[2], k1[3]);
}

// ---------------------------------------------------------------------------------------
// synthetic 64 B records (CPU twin: oracle orc_gen_records)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix_at(uint64_t seed, uint64_t k)
{
    uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_gen_records(const DevKeyTable *__restrict__ tab, int keysel,
                                                       uint8_t *__restrict__ recs, uint64_t stride, uint64_t n,
                                                       uint64_t seed, uint64_t first_index)
{
    fill_ttab<2>();
    fill_keys(tab);
    __syncthreads();
    const Lane l = lane_bases();
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BLOCK) {
        uint64_t i = first_index + j;
#if HFV_MUT_AUX == 5
        const uint64_t k = (uint32_t)(4 * i);
#else
        const uint64_t k = 4 * i;
#endif
        uint64_t r0 = splitmix_at(seed, k), r1 = splitmix_at(seed, k + 1);
        uint64_t r2 = splitmix_at(seed, k + 2), r3 = splitmix_at(seed, k + 3);
        uint32_t cons = (uint32_t)r0 & 1u;
        uint32_t beta = (uint32_t)(r0 >> 8) & 0xffffu;
        uint32_t ts_w = bswap((uint32_t)(r0 >> 32));
        uint32_t exp = (uint32_t)r1 & 0xffu;
        uint32_t ing = 1u + (uint32_t)((r1 >> 8) & 0xffffu) % 255u;
        uint32_t eg = 1u + (uint32_t)((r1 >> 24) & 0xffffu) % 255u;
        uint32_t hf0 = (exp << 8) | (bswap16(ing) << 16);
        uint32_t hf1 = bswap16(eg);
        uint32_t slot = keysel == HFV_KEYSEL_IFID ? ((cons ? ing : eg) & 0xffu) : 0u;
        const LdsKey key(slot);
        uint32_t w[4] = {bswap16(beta) << 16, ts_w, hf0, hf1}, s[4], tg4[4];
        cmac_general<2>(w, key, l, s);
        round_last_full<2>(s, key.row(10), l, tg4);
        uint32_t seg = cons ? beta : (beta ^ bswap16(tg4[0] & 0xffffu));
        uint64_t mac = (uint64_t)tg4[0] | ((uint64_t)(tg4[1] & 0xffffu) << 32);
        if ((r2 & 15u) == 0) mac ^= 1ull << ((r2 >> 4) % 48u);
        uint4 q0 = make_uint4(bswap((uint32_t)(r3 & 0xfffffu)), 0x04000f11u, 1u, 0x00ff0100u);
        uint4 q1 = make_uint4(0x10000000u, 0x00ff0100u, 0x11000000u, 0x0100000au);
        uint4 q2 = make_uint4(0x0200000au, 0x00100000u, cons | (bswap16(seg) << 16), ts_w);
        uint4 q3 = make_uint4(hf0, hf1 | ((uint32_t)mac << 16), (uint32_t)(mac >> 16), bswap((uint32_t)i));
#if HFV_MUT_AUX == 6
        uint4 *o = reinterpret_cast<uint4 *>(recs + j * 64);
#else
        uint4 *o = reinterpret_cast<uint4 *>(recs + j * stride);
#endif
        o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
constexpr int kBlockAux = 512;

// the test build's hfv_debug_aux_grid (g.aux_grid_cap; always 0 in the product library)
static inline unsigned aux_capped(const LaunchGeom &g, unsigned grid)
{
    return g.aux_grid_cap && g.aux_grid_cap < grid ? g.aux_grid_cap : grid;
}

int launch_verify_macinputs(const LaunchGeom &g, const DevKeyTable *tab, const void *mi, const uint64_t *expected,
                            const uint8_t *kidx, size_t n, uint64_t *bits, void *stream)
{
    unsigned grid = aux_capped(g, grid_for(n, kBlockAux, g.num_cus, 2));
    hipLaunchKernelGGL((k_macinputs<kModeMacinputs, kBlockAux>), dim3(grid), dim3(kBlockAux), 0, (hipStream_t)stream,
                       tab, (const uint4 *)mi, (const uint2 *)expected, kidx, (uint64_t)n, bits, (uint4 *)nullptr);
    return (int)hipGetLastError();
}

int launch_cmac_tags(const LaunchGeom &g, const DevKeyTable *tab, const void *mi, const uint8_t *kidx, size_t n,
                     void *tags, void *stream)
{
    unsigned grid = aux_capped(g, grid_for(n, kBlockAux, g.num_cus, 2));
    hipLaunchKernelGGL((k_macinputs<kModeTags, kBlockAux>), dim3(grid), dim3(kBlockAux), 0, (hipStream_t)stream, tab,
                       (const uint4 *)mi, (const uint2 *)nullptr, kidx, (uint64_t)n, (uint64_t *)nullptr,
                       (uint4 *)tags);
    return (int)hipGetLastError();
}

int launch_expand_keys(const uint8_t *raw, size_t n, hop_key *out, void *stream)
{
    unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_expand_keys, dim3(grid ? grid : 1), dim3(256), 0, (hipStream_t)stream, (const uint4 *)raw,
                       (uint64_t)n, out);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// record_verdict for the verify-only paths (xdp.c:54-70): per AS-ingress interface (the
// KEYSEL_IFID slot, IFID & 0xff, xdp.c:151-157) the packets that verified and the packets
// dropped as VERDICT_INVALID_HF, from the records and a verdict bitmap of either verify path.
// One lane per record; a block histogram in LDS, added to the u64 counters with one global
// atomic per non-zero bin.  HBM-bound: the three bytes it reads lie in the record's 64-byte line.
// ---------------------------------------------------------------------------------------
constexpr int kCountBlock = 512;
__global__ __launch_bounds__(kCountBlock) void k_count_verdicts(const uint8_t *__restrict__ recs, uint64_t stride,
                                                                uint64_t n, uint32_t inf_off, uint32_t hf_off,
                                                                const uint64_t *__restrict__ bits,
                                                                unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t h[512];
    for (uint32_t i = threadIdx.x; i < 512; i += kCountBlock) h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kCountBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kCountBlock) {
        const uint8_t *r = recs + i * stride;
        // Cons ? ConsIngress : ConsEgress, low byte of the big-endian field (rec_key_slot)
        const uint32_t slot = (r[inf_off] & 1u) ? r[hf_off + 3] : r[hf_off + 5];
#if HFV_MUT_AUX == 4
        const uint64_t first = (uint64_t)blockIdx.x * kCountBlock + threadIdx.x;
        const uint32_t pass = (uint32_t)(bits[first >> 6] >> (i & 63)) & 1u;
#else
        const uint32_t pass = (uint32_t)(bits[i >> 6] >> (i & 63)) & 1u;
#endif
        atomicAdd(&h[slot * 2 + (pass ^ 1u)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 512; i += kCountBlock)
        if (h[i]) atomicAdd(counters + i, (unsigned long long)h[i]);
}

int launch_count_verdicts(const LaunchGeom &g, const uint8_t *recs, size_t stride, size_t n, uint32_t inf_off,
                          uint32_t hf_off, const uint64_t *bits, uint64_t *counters, void *stream)
{
    unsigned grid = aux_capped(g, grid_for(n, kCountBlock, g.num_cus, 1));
    hipLaunchKernelGGL(k_count_verdicts, dim3(grid), dim3(kCountBlock), 0, (hipStream_t)stream, recs, (uint64_t)stride,
                       (uint64_t)n, inf_off, hf_off, bits, (unsigned long long *)counters);
    return (int)hipGetLastError();
}

int launch_gen_records(const LaunchGeom &g, const DevKeyTable *tab, int keysel, uint8_t *recs, size_t stride,
                       size_t n, uint64_t seed, uint64_t first_index, void *stream)
{
    uint64_t blocks = (n + kBlockAux - 1) / kBlockAux;
    uint64_t cap = (uint64_t)g.num_cus * 2;
    unsigned grid = aux_capped(g, (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap));
    hipLaunchKernelGGL((k_gen_records<kBlockAux>), dim3(grid), dim3(kBlockAux), 0, (hipStream_t)stream, tab, keysel,
                       recs, (uint64_t)stride, (uint64_t)n, seed, first_index);
    return (int)hipGetLastError();
}

}  // namespace hfv
