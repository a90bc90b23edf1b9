// hfv_frame_desc.h -- when a frame descriptor (struct hfv_frame_desc, include/scion_hfv.h) may be
// followed into the buffer it points into.  One rule for the host (hfv_frame_desc_ok, hfv_api.cpp)
// and the device (k_verify_frames_desc, hfv_frames_desc_kernel.hip), as hfv_frame_parse.h is shared.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HFV_DESC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HFV_DESC_HD inline
#endif

namespace hfv {

constexpr uint32_t kFrameDescMaxLen = 65535u;   // HFV_FRAME_DESC_MAX_LEN
constexpr int kFrameBadDesc = 255;              // HFV_FRAME_BAD_DESC

// The frame [addr, addr + len) lies inside [0, umem_bytes) and is no longer than a frame can be.
// addr + len is never formed, so nothing wraps; len == 0 is valid at every addr <= umem_bytes.
HFV_DESC_HD bool frame_desc_ok(uint64_t addr, uint32_t len, uint64_t umem_bytes)
{
    return len <= kFrameDescMaxLen && addr <= umem_bytes && (uint64_t)len <= umem_bytes - addr;
}

}  // namespace hfv
