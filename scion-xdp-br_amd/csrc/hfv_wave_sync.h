// hfv_wave_sync.h -- the wave-level LDS hand-over of the staging kernels (hfv_br_kernel.hip,
// hfv_frames_kernel.hip): rows one lane wrote are read by another lane of the same wave.
#pragma once
#include <hip/hip_runtime.h>

namespace hfv {

// Every LDS access of the wave before this point is done before any after it.  A wave runs in
// lockstep, so no s_barrier: the fences order the LDS queue (lgkmcnt), the barrier keeps the
// compiler from moving accesses across.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace hfv
