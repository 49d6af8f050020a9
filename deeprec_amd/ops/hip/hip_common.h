// hip_common.h — what every .hip translation unit of the extension shares:
// the torch / HIP includes, the current-stream accessor and the bf16 <->
// fp32 conversions on raw 16-bit patterns (the kernels carry bf16 as short).
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <cstdint>

// current-stream accessor (ROCm ATen name)
static inline hipStream_t current_hip_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// Grid size for a grid-stride elementwise kernel: enough blocks to keep the
// chip filled, capped at 65535.
// NOTE every kernel launched through this cap MUST grid-stride: a plain
// `if (i >= n) return` silently drops the tail past 65535 * block threads.
static inline int n_blocks(int64_t total, int block = 256) {
  int64_t b = (total + block - 1) / block;
  return (int)std::min<int64_t>(b, 65535);
}

static __device__ __forceinline__ float bf2f_u16(short u) {
  union {
    unsigned int i;
    float f;
  } cv;
  cv.i = ((unsigned int)(unsigned short)u) << 16;
  return cv.f;
}

// round-to-nearest-even; no NaN special case (a NaN with only low mantissa
// bits set rounds into infinity — callers that can see one handle it)
static __device__ __forceinline__ short f2bf_u16(float f) {
  union {
    float f;
    unsigned int i;
  } cv;
  cv.f = f;
  unsigned int lsb = (cv.i >> 16) & 1;
  cv.i += 0x7fff + lsb;
  return (short)(cv.i >> 16);
}
