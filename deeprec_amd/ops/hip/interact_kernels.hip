// interact_kernels.hip — the DLRM pair-dot interaction on MFMA for gfx950
// (CDNA4), D == 16 and F <= 32 feature rows. docs/KERNELS.md
// ("interact_kernels.hip") has the layouts in full.
//
// Per sample, with X the [F, 16] feature matrix padded to 32 zero rows:
//   forward   Z = X Xᵀ                one v_mfma_f32_32x32x16_bf16
//             out[p(i, j)] = bf(Z[i][j]), i < j < F,
//             p(i, j) = i F - i (i + 1) / 2 + (j - i - 1)
//   backward  dX = S X                two v_mfma_f32_16x16x32_bf16
//             S[i][j] = g[p(min, max)] for i != j, both < F, else 0
// With CAT the sample's row 0 is `bot` and rows 1.. are `emb`; the output
// row starts with the 16 bot values, and their incoming gradient is added
// to dX row 0 in fp32 before the one rounding.
//
//   k_interact_mfma_fwd<CAT>   operands straight from global memory into
//                              the fragment (A and B are the same
//                              registers), packed triangle staged in LDS
//   k_interact_mfma_bwd<CAT>   X staged row-major in LDS and read back
//                              transposed (ds_read_b64_tr_b16), S gathered
//                              from the grad row in LDS
//
// A wave owns IM_NS consecutive samples and nothing crosses waves: wave-
// level fences, no block barrier. The scalar kernels in dense_kernels.hip
// serve every other shape; the dispatch is in the wrappers there.

#include "hip_common.h"
#include "mfma_fwd.h"

namespace {

constexpr int IM_D = 16;
constexpr int IM_MAX_F = 32;
constexpr int IM_MAX_PPAD = 1024;  // bounds the forward's LDS rows
constexpr int IM_WAVES = 4;
#ifndef INTERACT_NS
#define INTERACT_NS 2
#endif
constexpr int IM_NS = INTERACT_NS;  // samples per wave, loads issued together

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x4 = __attribute__((ext_vector_type(4))) short;

// Orders one wave's LDS writes against its own later reads across lanes.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Transposed LDS read (rules in dense_kernels.hip: 8-byte aligned
// addresses, EXEC all ones, so only under wave-uniform control flow).
__device__ __forceinline__ bf16x4 lds_read_tr16(const short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

__device__ __forceinline__ int pair_index(int i, int j, int F) {  // i < j
  return i * F - ((i * (i + 1)) >> 1) + (j - i - 1);
}

// This lane's 16 bytes of sample b: row lane % 32, columns 8 (lane / 32)..
// The address is clamped into the operand (a bounds branch around the load
// would serialise the samples' loads); `ok` says whether the lane's row
// exists, and the caller replaces the value by zeros where it does not —
// by a select, the clamped source may hold anything.
template <bool CAT>
__device__ __forceinline__ const short* x_frag_ptr(const short* __restrict__ x0,
                                                   const short* __restrict__ emb,
                                                   int b, int B, int F,
                                                   int lane, bool& ok) {
  const int row = lane & 31;
  ok = b < B && row < F;
  const int64_t bc = min(b, B - 1);
  const int rc = min(row, F - 1);
  const int col = (lane >> 5) * 8;
  if (CAT)
    return rc == 0 ? x0 + bc * IM_D + col
                   : emb + (bc * (F - 1) + (rc - 1)) * IM_D + col;
  return x0 + (bc * F + rc) * IM_D + col;
}

// x0: bot [B, 16] (CAT) or feats [B, F, 16]; emb [B, F - 1, 16] (CAT only).
// out [B, R], R = (CAT ? 16 : 0) + P_pad, R % 8 == 0.
template <bool CAT>
__global__ __launch_bounds__(IM_WAVES * 64) void k_interact_mfma_fwd(
    const short* __restrict__ x0, const short* __restrict__ emb, int B, int F,
    int P_pad, short* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) short im_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b0 = (blockIdx.x * IM_WAVES + wave) * IM_NS;
  if (b0 >= B) return;
  constexpr int HEAD = CAT ? IM_D : 0;
  const int P = (F * (F - 1)) >> 1;
  const int R = HEAD + P_pad;
  short* rows = im_lds + wave * IM_NS * R;

  bf16x8 x[IM_NS];
  bool ok[IM_NS];
#pragma unroll
  for (int s = 0; s < IM_NS; ++s)
    x[s] = *reinterpret_cast<const bf16x8*>(
        x_frag_ptr<CAT>(x0, emb, b0 + s, B, F, lane, ok[s]));
  __builtin_amdgcn_sched_barrier(0);

  const int j = lane & 31;
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    const bf16x8 zero = {};
    const bf16x8 xs = ok[s] ? x[s] : zero;
    f32x16 z = {};
    z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xs, xs, z, 0, 0, 0);
    short* row = rows + s * R;
    if (CAT && j == 0)  // lanes 0 and 32 hold the bot row
      *reinterpret_cast<bf16x8*>(row + (lane >> 5) * 8) = xs;
    // accumulator r is Z[i][j], i = 8 (r / 4) + 4 (lane / 32) + r % 4
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (i < j && j < F) row[HEAD + pair_index(i, j, F)] = f2bf_u16(z[r]);
    }
    for (int p = P + lane; p < P_pad; p += 64) row[HEAD + p] = 0;
  }
  wave_lds_fence();
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    if (b0 + s >= B) break;
    const short* row = rows + s * R;
    short* dst = out + (int64_t)(b0 + s) * R;
    for (int c = lane * 8; c < R; c += 64 * 8)
      *reinterpret_cast<bf16x8*>(dst + c) =
          *reinterpret_cast<const bf16x8*>(row + c);
  }
}

// grad [B, R] as the forward's out; dx0: dbot (CAT) or dfeats; demb CAT only.
// LDS per sample: the X tile [32][16], then the grad row's first
// GL = HEAD + ceil8(P) elements (at most 64 16-byte chunks: one per lane).
// The chunk that holds column P - 1 may bring pad columns along; no pair
// index reaches them.
template <bool CAT>
__global__ __launch_bounds__(IM_WAVES * 64) void k_interact_mfma_bwd(
    const short* __restrict__ grad, const short* __restrict__ x0,
    const short* __restrict__ emb, int B, int F, int P_pad,
    short* __restrict__ dx0, short* __restrict__ demb) {
  extern __shared__ __attribute__((aligned(16))) short im_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b0 = (blockIdx.x * IM_WAVES + wave) * IM_NS;
  if (b0 >= B) return;
  constexpr int HEAD = CAT ? IM_D : 0;
  constexpr int TILE = 32 * IM_D;
  const int P = (F * (F - 1)) >> 1;
  const int R = HEAD + P_pad;
  const int GL = HEAD + ((P + 7) & ~7);
  const int SS = TILE + GL;
  short* base = im_lds + wave * IM_NS * SS;

  bf16x8 x[IM_NS], g[IM_NS];
  bool ok[IM_NS];
  const bool has_g = lane * 8 < GL;
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    x[s] = *reinterpret_cast<const bf16x8*>(
        x_frag_ptr<CAT>(x0, emb, b0 + s, B, F, lane, ok[s]));
    const int64_t bc = min(b0 + s, B - 1);
    g[s] = *reinterpret_cast<const bf16x8*>(grad + bc * R +
                                            (has_g ? lane * 8 : 0));
  }
  __builtin_amdgcn_sched_barrier(0);
  const int xoff = (lane & 31) * IM_D + (lane >> 5) * 8;
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    const bf16x8 zero = {};
    short* tile = base + s * SS;
    *reinterpret_cast<bf16x8*>(tile + xoff) = ok[s] ? x[s] : zero;
    if (has_g) *reinterpret_cast<bf16x8*>(tile + TILE + lane * 8) = g[s];
  }
  wave_lds_fence();

  // B fragment: X[8 (lane / 16) + e][lane % 16], e = 0..7, as two transposed
  // reads of 4 rows; within a 16-lane group lane 4 q + c addresses row q,
  // columns 4 c... The tile's 32-byte rows make each read's 8 rows one
  // contiguous 256-byte span: no bank conflict, no padding.
  const int kg = lane >> 4;
  const int troff = (8 * kg + ((lane >> 2) & 3)) * IM_D + 4 * (lane & 3);
  f32x4 acc[IM_NS][2];
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    const short* tile = base + s * SS;
    const short* gp = tile + TILE + HEAD;
    const bf16x4 lo = lds_read_tr16(tile + troff);
    const bf16x4 hi = lds_read_tr16(tile + troff + 4 * IM_D);
    const bf16x8 xt = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      // A fragment: S[i][j], i = 16 m + lane % 16, j = 8 (lane / 16) + e
      const int i = 16 * m + (lane & 15);
      bf16x8 sf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = 8 * kg + e;
        const int a = min(i, j), c = max(i, j);
        const bool on = a != c && c < F;
        const short v = gp[on ? pair_index(a, c, F) : 0];
        sf[e] = on ? v : (short)0;
      }
      const f32x4 zero = {};
      acc[s][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf, xt, zero, 0, 0, 0);
    }
  }
  // the X tiles are read; they now take dX (same [32][16] layout)
  wave_lds_fence();
  const int d = lane & 15;
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    short* tile = base + s * SS;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        // accumulator t is dX[i][d], i = 16 m + 4 (lane / 16) + t
        const int i = 16 * m + 4 * kg + t;
        float v = acc[s][m][t];
        if (CAT && i == 0) v += bf2f_u16(tile[TILE + d]);  // direct grad
        tile[i * IM_D + d] = f2bf_u16(v);
      }
  }
  wave_lds_fence();
  const int row = lane & 31;
  const int col = (lane >> 5) * 8;
#pragma unroll
  for (int s = 0; s < IM_NS; ++s) {
    const int64_t b = b0 + s;
    if (b >= B || row >= F) continue;
    const bf16x8 v =
        *reinterpret_cast<const bf16x8*>(base + s * SS + row * IM_D + col);
    short* dst;
    if (CAT)
      dst = row == 0 ? dx0 + b * IM_D + col
                     : demb + (b * (F - 1) + (row - 1)) * IM_D + col;
    else
      dst = dx0 + (b * F + row) * IM_D + col;
    *reinterpret_cast<bf16x8*>(dst) = v;
  }
}

int im_blocks(int B) {
  const int waves = (B + IM_NS - 1) / IM_NS;
  return (waves + IM_WAVES - 1) / IM_WAVES;
}

void check_aligned16(const void* p, const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(p) & 15) == 0,
              "interact (MFMA): ", name, " must be 16-byte aligned");
}

}  // namespace

// ---------------------- launchers (called from dense_kernels.hip) ---------

bool interact_mfma_eligible(int64_t F, int64_t D, int64_t p_pad) {
  return D == IM_D && F >= 2 && F <= IM_MAX_F && (p_pad & 7) == 0 &&
         p_pad >= F * (F - 1) / 2 && p_pad <= IM_MAX_PPAD;
}

// emb == nullptr: x0 is feats [B, F, 16]; else x0 is bot [B, 16] and emb
// [B, F - 1, 16], and out has the 16 bot columns in front.
void interact_mfma_fwd_launch(const short* x0, const short* emb, int B, int F,
                              int p_pad, short* out) {
  if (B == 0) return;
  check_aligned16(x0, emb ? "bot" : "feats");
  check_aligned16(emb, "emb");
  check_aligned16(out, "out");
  const int R = (emb ? IM_D : 0) + p_pad;
  const size_t lds = (size_t)IM_WAVES * IM_NS * R * sizeof(short);
  if (emb)
    k_interact_mfma_fwd<true><<<im_blocks(B), IM_WAVES * 64, lds,
                                current_hip_stream()>>>(x0, emb, B, F, p_pad,
                                                        out);
  else
    k_interact_mfma_fwd<false><<<im_blocks(B), IM_WAVES * 64, lds,
                                 current_hip_stream()>>>(x0, emb, B, F, p_pad,
                                                         out);
}

void interact_mfma_bwd_launch(const short* grad, const short* x0,
                              const short* emb, int B, int F, int p_pad,
                              short* dx0, short* demb) {
  if (B == 0) return;
  check_aligned16(grad, "grad");
  check_aligned16(x0, emb ? "bot" : "feats");
  check_aligned16(emb, "emb");
  check_aligned16(dx0, emb ? "dbot" : "dfeats");
  check_aligned16(demb, "demb");
  const int P = F * (F - 1) / 2;
  const int GL = (emb ? IM_D : 0) + ((P + 7) & ~7);
  const size_t lds =
      (size_t)IM_WAVES * IM_NS * (32 * IM_D + GL) * sizeof(short);
  if (emb)
    k_interact_mfma_bwd<true><<<im_blocks(B), IM_WAVES * 64, lds,
                                current_hip_stream()>>>(
        grad, x0, emb, B, F, p_pad, dx0, demb);
  else
    k_interact_mfma_bwd<false><<<im_blocks(B), IM_WAVES * 64, lds,
                                 current_hip_stream()>>>(
        grad, x0, emb, B, F, p_pad, dx0, demb);
}
