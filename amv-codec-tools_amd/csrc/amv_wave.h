// amv_wave.h -- what kernels share about a wave beyond its size (amv_segment.h: that header stays free of HIP).
#pragma once
#include <hip/hip_runtime.h>

#include "amv_segment.h"

namespace amv {

// the sum of v over the wave's kWave lanes, in every lane (all lanes must call it)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
    return v;
}

}  // namespace amv
