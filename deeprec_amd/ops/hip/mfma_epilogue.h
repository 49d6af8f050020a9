// mfma_epilogue.h — the element rules and the dX tile store of the MFMA
// linear kernels, shared by dense_kernels.hip and moe_kernels.hip so that a
// grouped-expert kernel and the per-layer kernel it replaces agree bit for
// bit. They hold per-lane bounds checks, so none of them may contain a
// transposed LDS read.
#pragma once

#include "mfma_fwd.h"

namespace {

// activation gradient of one element: g * act'(out), with out the saved
// bf16 activation; act 1=relu, 2=sigmoid. Shared by k_act_bwd and the dX
// epilogues so that the fused and the two-kernel forms agree bit for bit.
__device__ __forceinline__ short act_grad_u16(short g, short o, int act) {
  const float ov = bf2f_u16(o);
  if (act == 1) return ov > 0.0f ? g : (short)0;
  return f2bf_u16(bf2f_u16(g) * ov * (1.0f - ov));
}

// Strided fragment: element i = src[k0 + i][c] (column c of row-major src).
__device__ __forceinline__ bf16x8 load_frag_col(const short* __restrict__ src,
                                                int c, int k0, int rows,
                                                int cols) {
  bf16x8 out;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    short v = 0;
    int r = k0 + i;
    if (r < rows && c < cols) v = src[(int64_t)r * cols + c];
    out[i] = v;
  }
  return out;
}

// one forward element: act(acc + bias) rounded to bf16; act 1=relu (written
// as v < 0 -> 0 so that NaN passes through), 2=sigmoid
__device__ __forceinline__ short fwd_act_u16(float acc, float bv, int act) {
  float v = acc + bv;
  if (act == 1 && v < 0.0f) v = 0.0f;
  else if (act == 2) v = 1.0f / (1.0f + __expf(-v));
  return f2bf_u16(v);
}

// dX store of one wave's 16 x 64 accumulator tile at (m0, c0), kt live
// 16-column subtiles: round to bf16, then (prev_out set) the activation
// gradient of the layer below; bounded by M and K.
__device__ __forceinline__ void dx_store_tile(
    const f32x4 (&acc)[4], int lane, int m0, int c0, int kt, int M, int K,
    short* __restrict__ dX, const short* __restrict__ prev_out,
    int prev_act) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= kt) break;
    const int ck = c0 + t * 16 + (lane & 15);
    if (ck >= K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int cm = m0 + (lane >> 4) * 4 + i;
      if (cm >= M) continue;
      short v = f2bf_u16(acc[t][i]);
      if (prev_out)
        v = act_grad_u16(v, prev_out[(int64_t)cm * K + ck], prev_act);
      dX[(int64_t)cm * K + ck] = v;
    }
  }
}

}  // namespace
