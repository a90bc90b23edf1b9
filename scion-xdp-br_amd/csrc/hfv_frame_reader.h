// hfv_frame_reader.h -- the staged header window of the frame kernels (k_extract_records in
// hfv_frames_kernel.hip, k_verify_frames in hfv_frames_fused_kernel.hip) and the byte reader the
// parser (hfv_frame_parse.h) runs on there.  Only for the .hip units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// HFV_MUT_WINEDGE = 5 (`make winedge`, see hfv_br_kernel.hip): u32 takes a field across the window
// end from the row and its zeroed pad dword.  0 (the default, every product build): as written.
#ifndef HFV_MUT_WINEDGE
#define HFV_MUT_WINEDGE 0
#endif

namespace hfv {

constexpr int kFrWin = 128;              // staged bytes per frame
constexpr int kFrRow = kFrWin / 4 + 1;   // row pitch in dwords (odd)
constexpr int kFrC = kFrWin / 16;        // lanes (16-byte chunks) per staged frame

typedef uint32_t fr_v4u __attribute__((ext_vector_type(4)));
typedef uint32_t fr_v2u __attribute__((ext_vector_type(2)));

// Frame bytes for the parser: inside the window from the lane's LDS row, past it from the frame.
template <int WIN>
struct FrameReader {
    const uint32_t *row;
    const uint8_t *p;
    __device__ __forceinline__ uint32_t g8(int off) const { return p[off]; }
    __device__ __forceinline__ uint32_t g16(int off) const { return g8(off) | g8(off + 1) << 8; }
    __device__ __forceinline__ uint32_t u8(int off) const
    {
        if (WIN == 0 || off >= WIN) return g8(off);
        return reinterpret_cast<const uint8_t *>(row)[off];
    }
    __device__ __forceinline__ uint32_t u16(int off) const   // off even
    {
        if (WIN == 0 || off + 2 > WIN) return g16(off);
        return *reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(row) + off);
    }
    __device__ __forceinline__ uint32_t u32(int off) const
    {
        if (WIN == 0 || off + 4 > WIN + (HFV_MUT_WINEDGE == 5 ? 2 : 0)) return g16(off) | g16(off + 2) << 16;
        const int a = off >> 2;   // row[a + 1] is at most the pad dword (zeroed), and then shifted out
        const uint64_t two = (uint64_t)row[a + 1] << 32 | row[a];
        return (uint32_t)(two >> (8 * (off & 3)));
    }
};

}  // namespace hfv
