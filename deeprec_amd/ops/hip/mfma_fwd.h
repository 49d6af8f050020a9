// mfma_fwd.h — the forward GEMM's operand side, shared by the kernels that
// compute A[M,K] @ W[N,K]^T on v_mfma_f32_16x16x32_bf16 and differ only in
// their epilogue (dense_kernels.hip: activation; cross_kernels.hip: the
// DCNv2 cross update; moe_kernels.hip: grouped experts and the gate
// mixture). Fragment layouts per the CDNA4 ISA: A: row=lane%16,
// k=8*(lane/16)+i; B: col=lane%16, same k; D: col=lane%16,
// row=4*(lane/16)+i.
#pragma once

#include "hip_common.h"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// Load an 8-wide bf16 fragment row: src row-major [rows, cols], fragment
// element i = src[r][k0 + i]; ZERO-FILLED outside bounds.
__device__ __forceinline__ bf16x8 load_frag_row(const short* __restrict__ src,
                                                int r, int k0, int rows,
                                                int cols) {
  bf16x8 out;
  if (r < rows && k0 + 7 < cols) {
    const short* p = src + (int64_t)r * cols + k0;
    // 16B vector load
    out = *reinterpret_cast<const bf16x8*>(p);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      short v = 0;
      if (r < rows && k0 + i < cols) v = src[(int64_t)r * cols + k0 + i];
      out[i] = v;
    }
  }
  return out;
}

// ------------------------------------------------------------------
// K loop (fwd_accumulate). A wave's only latency hiding is its own loads in flight (the
// DLRM layers give a SIMD 0.5 to 4 waves), so the loop is built around
// that: the MT + 4 fragment loads of a 32-wide K step are unconditional
// 16-B loads from addresses that are always inside the operand, issued
// back to back, and the loads of step i+1 are issued before the MFMAs of
// step i (two register buffers, loop unrolled by two so that both are
// statically named). A bounds test around a load would make the compiler
// branch around it and drain vmcnt after it, one L2 round trip per
// fragment. Rows past M or N are instead read from the clamped last row
// and replaced by zeros with a select (never a multiply: the clamp source
// may hold NaN); waves whose 16*MT x 64 tile is interior (EDGE = false)
// skip clamp and select. The K tail (K % 32) is one more step: with
// K % 8 == 0 a lane's fragment is wholly inside or outside K, outside
// lanes read column 0 of their row and are zeroed by the same select;
// otherwise the element-wise load_frag_row. Each accumulator sees the
// same MFMAs in the same ascending-k order whatever the path.
// ------------------------------------------------------------------
template <int MT>
struct FwdStep {  // one K step of a wave's operands
  bf16x8 a[MT];
  bf16x8 b[4];
};

// 16-B fragment load without an alignment promise: W may start at an odd
// bf16 element, and rows are not 16-B aligned when K % 8 != 0
typedef bf16x8 bf16x8_u __attribute__((aligned(2)));

template <int MT, bool EDGE>
__device__ __forceinline__ void fwd_accumulate(const short* __restrict__ A,
                                               const short* __restrict__ W,
                                               int M, int N, int K, int m0,
                                               int n0, int lane,
                                               f32x4 (&acc)[MT][4]) {
  const int kgrp = (lane >> 4) * 8;
  // this lane's fragment rows at column kgrp, clamped into the operand
  const short* ap[MT];
  const short* bp[4];
  bool a_ok[MT], b_ok[4];
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    const int row = m0 + r * 16 + (lane & 15);
    a_ok[r] = !EDGE || row < M;
    ap[r] = A + (int64_t)(EDGE ? min(row, M - 1) : row) * K + kgrp;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = n0 + t * 16 + (lane & 15);
    b_ok[t] = !EDGE || row < N;
    bp[t] = W + (int64_t)(EDGE ? min(row, N - 1) : row) * K + kgrp;
  }
  auto load = [&](FwdStep<MT>& s, int koff) {
#pragma unroll
    for (int r = 0; r < MT; ++r)
      s.a[r] = *reinterpret_cast<const bf16x8_u*>(ap[r] + koff);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      s.b[t] = *reinterpret_cast<const bf16x8_u*>(bp[t] + koff);
    // keep the scheduler from sinking a step's loads below the MFMAs
    // they are meant to overlap, or its selects in between the loads
    __builtin_amdgcn_sched_barrier(0);
  };
  // zero the fragments of rows past M / N and (kin false) columns past K
  auto zero_fill = [&](FwdStep<MT>& s, bool kin) {
    const bf16x8 zero = {};
#pragma unroll
    for (int r = 0; r < MT; ++r) s.a[r] = (a_ok[r] && kin) ? s.a[r] : zero;
#pragma unroll
    for (int t = 0; t < 4; ++t) s.b[t] = (b_ok[t] && kin) ? s.b[t] : zero;
  };
  auto mfma = [&](const FwdStep<MT>& s) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < MT; ++r)
        acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            s.a[r], s.b[t], acc[r][t], 0, 0, 0);
  };
  auto step = [&](FwdStep<MT>& s) {
    if (EDGE) zero_fill(s, true);
    mfma(s);
  };

  const int nfull = K / 32;
  FwdStep<MT> s0, s1;
  if (nfull > 0) {
    load(s0, 0);
    int i = 0;  // s0 holds step i
    for (; i + 2 < nfull; i += 2) {
      load(s1, (i + 1) * 32);
      step(s0);
      load(s0, (i + 2) * 32);
      step(s1);
    }
    if (i + 2 == nfull) {  // two steps left, nothing to prefetch after them
      load(s1, (i + 1) * 32);
      step(s0);
      step(s1);
    } else {
      step(s0);
    }
  }
  const int kt = nfull * 32;
  if (kt == K) return;
  if ((K & 7) == 0) {
    const bool kin = kt + kgrp < K;
    load(s0, kin ? kt : -kgrp);
    zero_fill(s0, kin);
  } else {
#pragma unroll
    for (int r = 0; r < MT; ++r)
      s0.a[r] = load_frag_row(A, m0 + r * 16 + (lane & 15), kt + kgrp, M, K);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      s0.b[t] = load_frag_row(W, n0 + t * 16 + (lane & 15), kt + kgrp, N, K);
  }
  mfma(s0);
}

}  // namespace
