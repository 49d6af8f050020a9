// mask_kernels.hip — the MaskNet mask block for gfx950 (CDNA4 MFMA):
//   h' = relu(LN((mask * h) W^T + b))
// docs/KERNELS.md ("mask_kernels.hip") has the whole numerical contract:
//   p  = bf(float(mask) * float(h))          one rounding of the exact product
//   v  = p · bf(W)^T + b                     fp32 MFMA accumulation
//   mean = sum(v) / N, d = v - mean, var = sum(d^2) / N       two passes
//   rstd = rsqrt(var + eps), y = bf(relu(d * rstd * gamma + beta))
// and backward, from the saved z = bf(v), (mean, rstd) and y:
//   g = y > 0 ? dy : 0, xh = (z - mean) rstd, gg = g gamma
//   dz = bf((gg - mean(gg) - xh mean(gg xh)) rstd)
//   dgamma = sum_rows g xh, dbeta = sum_rows g
//   dp = dz · bf(W) (linear_dx), dW = dz^T · p (linear_dw)
//   dmask = bf(dp * h), dh = bf(dp * mask)
//
//   k_maskblock_fwd   the GEMM whose A operand is formed in registers from
//                     two tensors, with the LayerNorm and the ReLU on the
//                     accumulators: a block owns complete rows
//   k_ln_relu_bwd     one wave per row
//   k_mask_split_bwd  element-wise

#include "hip_common.h"
#include "mfma_fwd.h"

namespace py = pybind11;

namespace {

constexpr int MB_MAX_N = 256;  // 4 waves x 64 columns: a block owns a row

typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16x4 bf16x4_u __attribute__((aligned(2)));

// p = bf(m * h): the fp32 product of two bf16 values is exact, so this is
// one rounding of the exact product (what torch's fp32 multiply and cast
// give).
__device__ __forceinline__ bf16x8 mask_mul(bf16x8 m, bf16x8 h) {
  bf16x8 p;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    p[i] = f2bf_u16(bf2f_u16(m[i]) * bf2f_u16(h[i]));
  return p;
}

template <int MT>
struct MaskStep {  // one K step of a wave's operands
  bf16x8 m[MT];
  bf16x8 h[MT];
  bf16x8 b[4];
};

// ------------------------------------------------------------------
// acc += (Mk * H)[16 MT rows at m0, K] @ W[64 rows at n0, K]^T. The K loop
// of fwd_accumulate (mfma_fwd.h) with a two-tensor A side: unconditional
// 16-B loads from addresses clamped into the operands, the loads of step
// i + 1 issued before the MFMAs of step i, rows past M or N and columns
// past K replaced by zeros with a select after the product (the clamp
// source may hold anything), the K % 8 != 0 tail element by element. Each
// accumulator sees its MFMAs in ascending k whatever the path. P != null
// (wave-uniform): the wave also stores its A fragments to P[M, K].
// ------------------------------------------------------------------
template <int MT, bool EDGE>
__device__ __forceinline__ void mask_accumulate(
    const short* __restrict__ Mk, const short* __restrict__ H,
    const short* __restrict__ W, int M, int N, int K, int m0, int n0,
    int lane, short* __restrict__ P, f32x4 (&acc)[MT][4]) {
  const int kgrp = (lane >> 4) * 8;
  int64_t ao[MT];  // offset of this lane's fragment row at column kgrp
  const short* bp[4];
  bool a_ok[MT], b_ok[4];
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    const int row = m0 + r * 16 + (lane & 15);
    a_ok[r] = !EDGE || row < M;
    ao[r] = (int64_t)(EDGE ? min(row, M - 1) : row) * K + kgrp;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = n0 + t * 16 + (lane & 15);
    b_ok[t] = !EDGE || row < N;
    bp[t] = W + (int64_t)(EDGE ? min(row, N - 1) : row) * K + kgrp;
  }
  const bf16x8 zero = {};
  auto load = [&](MaskStep<MT>& s, int koff) {
#pragma unroll
    for (int r = 0; r < MT; ++r) {
      s.m[r] = *reinterpret_cast<const bf16x8_u*>(Mk + ao[r] + koff);
      s.h[r] = *reinterpret_cast<const bf16x8_u*>(H + ao[r] + koff);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
      s.b[t] = *reinterpret_cast<const bf16x8_u*>(bp[t] + koff);
    // keep a step's loads together and above the MFMAs they overlap
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mfma = [&](const bf16x8 (&a)[MT], const MaskStep<MT>& s) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < MT; ++r)
        acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[r], s.b[t], acc[r][t], 0, 0, 0);
  };
  // kin: this lane's fragment lies inside K (always, in a full step);
  // sel: the step needs its selects (an edge tile, or the K tail)
  auto step = [&](MaskStep<MT>& s, int koff, bool kin, bool sel) {
    bf16x8 a[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) {
      a[r] = mask_mul(s.m[r], s.h[r]);
      if (sel) a[r] = (a_ok[r] && kin) ? a[r] : zero;
    }
    if (sel) {
#pragma unroll
      for (int t = 0; t < 4; ++t) s.b[t] = (b_ok[t] && kin) ? s.b[t] : zero;
    }
    if (P) {
#pragma unroll
      for (int r = 0; r < MT; ++r)
        if (a_ok[r] && kin)
          *reinterpret_cast<bf16x8_u*>(P + ao[r] + koff) = a[r];
    }
    mfma(a, s);
  };

  const int nfull = K / 32;
  MaskStep<MT> s0, s1;
  if (nfull > 0) {
    load(s0, 0);
    int i = 0;  // s0 holds step i
    for (; i + 2 < nfull; i += 2) {
      load(s1, (i + 1) * 32);
      step(s0, i * 32, true, EDGE);
      load(s0, (i + 2) * 32);
      step(s1, (i + 1) * 32, true, EDGE);
    }
    if (i + 2 == nfull) {  // two steps left, nothing to prefetch after them
      load(s1, (i + 1) * 32);
      step(s0, i * 32, true, EDGE);
      step(s1, (i + 1) * 32, true, EDGE);
    } else {
      step(s0, i * 32, true, EDGE);
    }
  }
  const int kt = nfull * 32;
  if (kt == K) return;
  if ((K & 7) == 0) {
    // a lane's fragment is wholly inside or outside K; outside lanes read
    // column 0 of their row and are zeroed by the select
    const bool kin = kt + kgrp < K;
    load(s0, kin ? kt : -kgrp);
    step(s0, kt, kin, true);
    return;
  }
  bf16x8 a[MT];
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    const int row = m0 + r * 16 + (lane & 15);
    a[r] = mask_mul(load_frag_row(Mk, row, kt + kgrp, M, K),
                    load_frag_row(H, row, kt + kgrp, M, K));
    if (P && row < M) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (kt + kgrp + i < K) P[(int64_t)row * K + kt + kgrp + i] = a[r][i];
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
    s0.b[t] = load_frag_row(W, n0 + t * 16 + (lane & 15), kt + kgrp, N, K);
  mfma(a, s0);
}

// Orders one wave's LDS writes against its own later reads across lanes.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Store one wave's 16 x 64 tile of bf16 values (D layout: v[t][i] is column
// n0 + 16 t + lane%16, row m0 + 4*(lane/16) + i) into C[M, N]: a full tile
// through the wave's own LDS stage as 128-B row bursts, a ragged one
// element-wise within M and N.
__device__ __forceinline__ void store_tile_u16(const short (&v)[4][4],
                                               int lane, int m0, int n0,
                                               int M, int N,
                                               short* __restrict__ C,
                                               short (*stage)[72]) {
  if (n0 + 64 <= N && m0 + 16 <= M && (N & 7) == 0) {  // wave-uniform
    wave_lds_fence();  // the stage's previous reads are done
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        stage[(lane >> 4) * 4 + i][t * 16 + (lane & 15)] = v[t][i];
    wave_lds_fence();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int row = half * 8 + (lane >> 3);
      const int c8 = (lane & 7) * 8;
      const bf16x8 vreg = *reinterpret_cast<const bf16x8*>(&stage[row][c8]);
      *reinterpret_cast<bf16x8*>(C + (int64_t)(m0 + row) * N + n0 + c8) =
          vreg;
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cn = n0 + t * 16 + (lane & 15);
    if (cn >= N) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cm = m0 + (lane >> 4) * 4 + i;
      if (cm >= M) continue;
      C[(int64_t)cm * N + cn] = v[t][i];
    }
  }
}

// Sum over the 16 lanes that hold one accumulator row (lanes of equal
// lane/16): an xor butterfly, after which all 16 hold the same bits.
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int mask = 1; mask < 16; mask <<= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

// ------------------------------------------------------------------
// y = relu(LN((Mk * H) @ W^T + bias)). A block of 4 waves owns 16 MT rows
// and all N <= 256 columns; wave w owns columns 64 w .. 64 w + 63 (D
// layout: lane -> column lane%16 of each of its 4 column tiles, rows
// 4*(lane/16) + i). A wave whose columns lie past N runs no K loop and
// contributes zeros, but reaches both barriers.
// Row statistics on the fp32 accumulators: per lane the sum over its live
// columns in ascending tile order, the butterfly over the row's 16 lanes,
// one partial per (wave, row) in LDS, summed by every lane in wave order —
// a fixed order, so the result is the same from run to run.
// save: z = bf(v), stats = (mean, rstd) and p = bf(Mk * H) are stored too;
// p and stats by wave 0 alone.
// ------------------------------------------------------------------
template <int MT>
__global__ void __launch_bounds__(256) k_maskblock_fwd(
    const short* __restrict__ Mk, const short* __restrict__ H,
    const short* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, int M,
    int N, int K, float eps, short* __restrict__ Y, short* __restrict__ Z,
    float* __restrict__ stats, short* __restrict__ P) {
  __shared__ alignas(16) short cstage[4][16][72];  // 64 + 8: bank de-phase
  __shared__ float red[2][4][16 * MT];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16 * MT;
  const int n0 = wave * 64;
  const int cl = lane & 15, rq = (lane >> 4) * 4;

  f32x4 acc[MT][4] = {};
  if (n0 < N) {  // wave-uniform
    short* pw = wave == 0 ? P : nullptr;
    if (m0 + 16 * MT <= M && n0 + 64 <= N)
      mask_accumulate<MT, false>(Mk, H, W, M, N, K, m0, n0, lane, pw, acc);
    else
      mask_accumulate<MT, true>(Mk, H, W, M, N, K, m0, n0, lane, pw, acc);
  }

  bool c_ok[4];
  float gm[4], bt[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cn = n0 + t * 16 + cl;
    c_ok[t] = cn < N;
    const int cc = c_ok[t] ? cn : 0;
    const float bv = bias[cc];
    gm[t] = gamma[cc];
    bt[t] = beta[cc];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[r][t][i] += bv;
  }
  if (Z && n0 < N) {
#pragma unroll
    for (int r = 0; r < MT; ++r) {
      short v[4][4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[t][i] = f2bf_u16(acc[r][t][i]);
      store_tile_u16(v, lane, m0 + r * 16, n0, M, N, Z, cstage[wave]);
    }
  }

  // pass 1: the mean
#pragma unroll
  for (int r = 0; r < MT; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) s += c_ok[t] ? acc[r][t][i] : 0.0f;
      s = row16_sum(s);
      if (cl == 0) red[0][wave][r * 16 + rq + i] = s;
    }
  __syncthreads();
  float mean[MT][4], rstd[MT][4];
#pragma unroll
  for (int r = 0; r < MT; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = r * 16 + rq + i;
      mean[r][i] = (((red[0][0][lr] + red[0][1][lr]) + red[0][2][lr]) +
                    red[0][3][lr]) / (float)N;
    }
  // pass 2: the variance of d = v - mean
#pragma unroll
  for (int r = 0; r < MT; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float d = acc[r][t][i] - mean[r][i];
        acc[r][t][i] = d;
        s += c_ok[t] ? d * d : 0.0f;
      }
      s = row16_sum(s);
      if (cl == 0) red[1][wave][r * 16 + rq + i] = s;
    }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < MT; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = r * 16 + rq + i;
      const float var = (((red[1][0][lr] + red[1][1][lr]) + red[1][2][lr]) +
                         red[1][3][lr]) / (float)N;
      rstd[r][i] = rsqrtf(var + eps);
      const int row = m0 + lr;
      if (stats && wave == 0 && cl == 0 && row < M) {
        stats[(int64_t)row * 2] = mean[r][i];
        stats[(int64_t)row * 2 + 1] = rstd[r][i];
      }
    }
  if (n0 >= N) return;
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    short v[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float yv = acc[r][t][i] * rstd[r][i] * gm[t] + bt[t];
        if (yv < 0.0f) yv = 0.0f;  // written so that NaN passes through
        v[t][i] = f2bf_u16(yv);
      }
    store_tile_u16(v, lane, m0 + r * 16, n0, M, N, Y, cstage[wave]);
  }
}

// 4 contiguous bf16 of a row of width N starting at column c, zeros past N
__device__ __forceinline__ bf16x4 load_row4(const short* __restrict__ row,
                                            int c, int N) {
  if (c + 3 < N) return *reinterpret_cast<const bf16x4_u*>(row + c);
  bf16x4 out = {};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c + j < N) out[j] = row[c + j];
  return out;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) v += __shfl_xor(v, mask, 64);
  return v;
}

constexpr int LNB_WAVES = 4;          // rows in flight per block
constexpr int LNB_ROWS_PER_WAVE = 8;  // amortizes the dgamma / dbeta merge
constexpr int LNB_MAX_BLOCKS = 1024;

// ------------------------------------------------------------------
// Backward of y = relu(LN(z)) for N <= 256. One wave per row, grid-stride
// over rows; lane l holds columns 4 l .. 4 l + 3. dgamma / dbeta partials
// stay in the lane's registers across its rows, the block's 4 waves merge
// through LDS in wave order, the blocks merge with fp32 atomics into the
// zero-filled output. Launch: min(ceil(M / 32), 1024) blocks of 4 waves, so
// one dgamma element is a chain of ceil(M / (4 blocks)) + 4 + blocks
// additions.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(64 * LNB_WAVES) k_ln_relu_bwd(
    const short* __restrict__ dy, const short* __restrict__ y,
    const short* __restrict__ z, const float* __restrict__ stats,
    const float* __restrict__ gamma, int M, int N, short* __restrict__ dz,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float part[2][LNB_WAVES][MB_MAX_N];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c0 = lane * 4;
  float gm[4], pg[4] = {}, pb[4] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) gm[j] = c0 + j < N ? gamma[c0 + j] : 0.0f;
  const float inv_n = 1.0f / (float)N;
  for (int row = blockIdx.x * LNB_WAVES + wave; row < M;
       row += gridDim.x * LNB_WAVES) {
    const int64_t o = (int64_t)row * N;
    const bf16x4 dyv = load_row4(dy + o, c0, N);
    const bf16x4 yv = load_row4(y + o, c0, N);
    const bf16x4 zv = load_row4(z + o, c0, N);
    const float mean = stats[(int64_t)row * 2];
    const float rstd = stats[(int64_t)row * 2 + 1];
    float xh[4], gg[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = c0 + j < N;
      const float g = bf2f_u16(yv[j]) > 0.0f ? bf2f_u16(dyv[j]) : 0.0f;
      xh[j] = live ? (bf2f_u16(zv[j]) - mean) * rstd : 0.0f;
      gg[j] = g * gm[j];
      s1 += gg[j];
      s2 += gg[j] * xh[j];
      pg[j] += g * xh[j];
      pb[j] += g;
    }
    s1 = wave_sum(s1) * inv_n;
    s2 = wave_sum(s2) * inv_n;
    bf16x4 dzv;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      dzv[j] = f2bf_u16((gg[j] - s1 - xh[j] * s2) * rstd);
    if (c0 + 3 < N) {
      *reinterpret_cast<bf16x4_u*>(dz + o + c0) = dzv;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < N) dz[o + c0 + j] = dzv[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    part[0][wave][c0 + j] = pg[j];
    part[1][wave][c0 + j] = pb[j];
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < N) {
    float sg = part[0][0][c], sb = part[1][0][c];
#pragma unroll
    for (int w = 1; w < LNB_WAVES; ++w) {
      sg += part[0][w][c];
      sb += part[1][w][c];
    }
    atomicAdd(&dgamma[c], sg);
    atomicAdd(&dbeta[c], sb);
  }
}

__global__ void k_zero_small(float* __restrict__ p, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0.0f;
}

// ------------------------------------------------------------------
// dm = bf(dp * h), dh = bf(dp * m) over n elements, 8 per thread and step
// (16-B accesses), scalar tail. Grid-stride.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mask_split_bwd(
    const short* __restrict__ dp, const short* __restrict__ m,
    const short* __restrict__ h, short* __restrict__ dm,
    short* __restrict__ dh, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n8 = n / 8;
  for (int64_t v = tid; v < n8; v += nthreads) {
    const bf16x8 g = *reinterpret_cast<const bf16x8_u*>(dp + v * 8);
    const bf16x8 mv = *reinterpret_cast<const bf16x8_u*>(m + v * 8);
    const bf16x8 hv = *reinterpret_cast<const bf16x8_u*>(h + v * 8);
    *reinterpret_cast<bf16x8_u*>(dm + v * 8) = mask_mul(g, hv);
    *reinterpret_cast<bf16x8_u*>(dh + v * 8) = mask_mul(g, mv);
  }
  for (int64_t p = n8 * 8 + tid; p < n; p += nthreads) {
    const float g = bf2f_u16(dp[p]);
    dm[p] = f2bf_u16(g * bf2f_u16(h[p]));
    dh[p] = f2bf_u16(g * bf2f_u16(m[p]));
  }
}

}  // namespace

// ---------------------- host wrappers ----------------------

static const short* bf_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr<at::BFloat16>());
}
static short* bf_ptr_mut(torch::Tensor& t) {
  return reinterpret_cast<short*>(t.data_ptr<at::BFloat16>());
}

// The kernels index their operands as dense row-major matrices of one
// dtype; anything else is rejected before a launch.
static void check_matrix(const torch::Tensor& t, c10::ScalarType dtype,
                         const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.dim() == 2, op, ": ", name, " must be 2-D, got ", t.dim(),
              "-D");
  TORCH_CHECK(t.scalar_type() == dtype, op, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name,
              " must be contiguous (row-major)");
}

static void check_operand(const torch::Tensor& t, c10::ScalarType dtype,
                          int64_t rows, int64_t cols, const char* op,
                          const char* name) {
  check_matrix(t, dtype, op, name);
  TORCH_CHECK(t.size(0) == rows && t.size(1) == cols, op, ": ", name,
              " is [", t.size(0), ",", t.size(1), "], expected [", rows, ",",
              cols, "]");
}

static void check_vector(const torch::Tensor& t, int64_t n, const char* op,
                         const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.dim() == 1 && t.numel() == n && t.is_contiguous(),
              op, ": ", name, " must be a contiguous fp32 GPU vector of ", n);
}

static void check_width(const char* op, int64_t N) {
  TORCH_CHECK(N >= 1 && N <= MB_MAX_N, op, ": the row width N must be in [1, ",
              MB_MAX_N, "], got ", N);
}

static void check_extent(const char* op, int64_t M, int64_t cols) {
  TORCH_CHECK(M * cols < (1LL << 31) && M < (1 << 30), op,
              ": M and M*cols must stay below 2^31");
}

static void check_one_device(
    const char* op, std::initializer_list<const torch::Tensor*> ts) {
  const auto dev = (*ts.begin())->device();
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->device() == dev, op,
                ": all operands must be on one device, got ", t->device(),
                " and ", dev);
}

// y = relu(LN((m * h) @ w^T + bias)); with save also z = bf(pre-LN),
// stats = (mean, rstd) per row and p = bf(m * h), else three empty tensors.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
maskblock_fwd(torch::Tensor m, torch::Tensor h, torch::Tensor w,
              torch::Tensor bias, torch::Tensor gamma, torch::Tensor beta,
              double eps, bool save, int64_t variant) {
  const char* op = "maskblock_fwd";
  TORCH_CHECK(variant >= -1 && variant <= 1, op, ": variant must be -1 "
              "(automatic), 0 (MT=1) or 1 (MT=2), got ", variant);
  check_matrix(m, torch::kBFloat16, op, "m");
  check_matrix(w, torch::kBFloat16, op, "w");
  const int64_t M = m.size(0), K = m.size(1), N = w.size(0);
  check_operand(h, torch::kBFloat16, M, K, op, "h");
  TORCH_CHECK(w.size(1) == K, op, ": m is [M,", K, "] but w is [N,",
              w.size(1), "]");
  check_width(op, N);
  TORCH_CHECK(K >= 1, op, ": empty weight");
  check_vector(bias, N, op, "bias");
  check_vector(gamma, N, op, "gamma");
  check_vector(beta, N, op, "beta");
  check_extent(op, M, std::max(K, N));
  check_one_device(op, {&m, &h, &w, &bias, &gamma, &beta});
  auto y = torch::empty({M, N}, m.options());
  auto z = torch::empty({save ? M : 0, N}, m.options());
  auto stats =
      torch::empty({save ? M : 0, 2}, m.options().dtype(torch::kFloat32));
  auto p = torch::empty({save ? M : 0, K}, m.options());
  if (M == 0) return {y, z, stats, p};
#define MASKBLOCK_FWD(MT)                                                   \
  k_maskblock_fwd<MT><<<(int)((M + 16 * MT - 1) / (16 * MT)), 256, 0,       \
                        current_hip_stream()>>>(                            \
      bf_ptr(m), bf_ptr(h), bf_ptr(w), bias.data_ptr<float>(),              \
      gamma.data_ptr<float>(), beta.data_ptr<float>(), (int)M, (int)N,      \
      (int)K, (float)eps, bf_ptr_mut(y), save ? bf_ptr_mut(z) : nullptr,    \
      save ? stats.data_ptr<float>() : nullptr,                             \
      save ? bf_ptr_mut(p) : nullptr)
  // -1, 1: MT = 2 measured faster at the model's shapes (8192 x 256 x 429:
  // 40.9 against 51.5 us; profiles/PERF_LOG.md, "Fused mask blocks")
  if (variant == 0) MASKBLOCK_FWD(1);
  else MASKBLOCK_FWD(2);
#undef MASKBLOCK_FWD
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {y, z, stats, p};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ln_relu_bwd(
    torch::Tensor dy, torch::Tensor y, torch::Tensor z, torch::Tensor stats,
    torch::Tensor gamma) {
  const char* op = "ln_relu_bwd";
  check_matrix(dy, torch::kBFloat16, op, "dy");
  const int64_t M = dy.size(0), N = dy.size(1);
  check_width(op, N);
  check_operand(y, torch::kBFloat16, M, N, op, "y");
  check_operand(z, torch::kBFloat16, M, N, op, "z");
  check_operand(stats, torch::kFloat32, M, 2, op, "stats");
  check_vector(gamma, N, op, "gamma");
  check_extent(op, M, N);
  check_one_device(op, {&dy, &y, &z, &stats, &gamma});
  auto dz = torch::empty_like(dy);
  auto dgb = torch::empty({2, N}, gamma.options());
  auto stream = current_hip_stream();
  // a fill kernel, not a memset: memset nodes do not replay in a captured
  // graph
  k_zero_small<<<1, 256, 0, stream>>>(dgb.data_ptr<float>(), (int)(2 * N));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if (M > 0) {
    const int per_block = LNB_WAVES * LNB_ROWS_PER_WAVE;
    const int blocks = (int)std::min<int64_t>((M + per_block - 1) / per_block,
                                              LNB_MAX_BLOCKS);
    k_ln_relu_bwd<<<blocks, 64 * LNB_WAVES, 0, stream>>>(
        bf_ptr(dy), bf_ptr(y), bf_ptr(z), stats.data_ptr<float>(),
        gamma.data_ptr<float>(), (int)M, (int)N, bf_ptr_mut(dz),
        dgb.data_ptr<float>(), dgb.data_ptr<float>() + N);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {dz, dgb.select(0, 0), dgb.select(0, 1)};
}

std::tuple<torch::Tensor, torch::Tensor> mask_split_bwd(torch::Tensor dp,
                                                        torch::Tensor m,
                                                        torch::Tensor h) {
  const char* op = "mask_split_bwd";
  check_matrix(dp, torch::kBFloat16, op, "dp");
  const int64_t M = dp.size(0), K = dp.size(1);
  check_operand(m, torch::kBFloat16, M, K, op, "m");
  check_operand(h, torch::kBFloat16, M, K, op, "h");
  check_one_device(op, {&dp, &m, &h});
  auto dm = torch::empty_like(dp);
  auto dh = torch::empty_like(dp);
  const int64_t n = M * K;
  if (n == 0) return {dm, dh};
  k_mask_split_bwd<<<n_blocks((n + 7) / 8), 256, 0, current_hip_stream()>>>(
      bf_ptr(dp), bf_ptr(m), bf_ptr(h), bf_ptr_mut(dm), bf_ptr_mut(dh), n);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dm, dh};
}

void register_mask(py::module_& mod) {
  mod.def("maskblock_fwd", &maskblock_fwd, py::arg("m"), py::arg("h"),
          py::arg("w"), py::arg("bias"), py::arg("gamma"), py::arg("beta"),
          py::arg("eps"), py::arg("save"), py::arg("variant") = -1);
  mod.def("ln_relu_bwd", &ln_relu_bwd, py::arg("dy"), py::arg("y"),
          py::arg("z"), py::arg("stats"), py::arg("gamma"));
  mod.def("mask_split_bwd", &mask_split_bwd, py::arg("dp"), py::arg("m"),
          py::arg("h"));
}
