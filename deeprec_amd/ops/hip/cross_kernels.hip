// cross_kernels.hip — DCNv2 cross layers for gfx950 (CDNA4 MFMA).
//
// A cross layer is x_{l+1} = x0 * u_l + x_l with u_l = W_l x_l + b_l, or,
// low rank, u_l = U_l (V_l x_l) + b_l. The residual stream x and its
// gradient stay fp32; the GEMM operands are bf16 (docs/KERNELS.md, "Cross
// layers", has the whole numerical contract):
//   a_l = bf(x_l)
//   u_l = a_l · bf(W_l)^T + b_l                    fp32 MFMA accumulation
//   t_l = bf(a_l · bf(V_l)^T), u_l = t_l · bf(U_l)^T + b_l     (low rank)
//   x_{l+1} = fmaf(x0, u_l, x_l)                   one rounding
// and backward, given g = dL/dx_{l+1}:
//   du = bf(g * x0), dx0 = fmaf(g, float(bf(u_l)), dx0)
//   g_l = g + du · bf(W_l)                                  (full matrix)
//   dt = bf(du · bf(U_l)), g_l = g + dt · bf(V_l)           (low rank)
// The weight gradients are plain linear_dw calls on du, dt, a_l and t_l.
//
//   k_cross_fwd     a GEMM with the cross epilogue; the operand side is the
//                   linear forward's K loop (mfma_fwd.h)
//   k_cross_dx      the same GEMM on du and W^T with the epilogue acc + g
//   k_cross_du      the elementwise step in front of k_cross_dx / dW
//   k_cross_lr_bwd  the data gradient of a low-rank layer in one launch:
//                   du is formed in registers as the A fragment, dt stays
//                   in the wave's LDS tile
// The forward of a low-rank layer is linear_fwd followed by k_cross_fwd: a
// one-launch forward measured no faster (profiles/PERF_LOG.md).

#include "hip_common.h"
#include "mfma_fwd.h"

namespace py = pybind11;

namespace {

// 16-B fp32 access without an alignment promise (rows of an odd D)
typedef f32x4 f32x4_u __attribute__((aligned(4)));

// Cross epilogue of one 16 x 16 accumulator tile at (m0, n0), D layout
// (col = lane%16, row = 4*(lane/16) + i), bounded by M and N. Per row 16
// lanes touch 64 contiguous bytes of each fp32 operand.
__device__ __forceinline__ void cross_store(
    f32x4 acc, int lane, int m0, int n0, int M, int N,
    const float* __restrict__ bias, const float* __restrict__ x0,
    const float* __restrict__ x, float* __restrict__ xn,
    short* __restrict__ xn16, short* __restrict__ u16) {
  const int cn = n0 + (lane & 15);
  if (cn >= N) return;
  const float bv = bias[cn];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cm = m0 + (lane >> 4) * 4 + i;
    if (cm >= M) continue;
    const int64_t o = (int64_t)cm * N + cn;
    const float u = acc[i] + bv;
    const float xv = fmaf(x0[o], u, x[o]);
    xn[o] = xv;
    xn16[o] = f2bf_u16(xv);
    if (u16) u16[o] = f2bf_u16(u);
  }
}

// Data-gradient epilogue of the same tile: g_prev = acc + g, fp32.
__device__ __forceinline__ void dx_add_store(f32x4 acc, int lane, int m0,
                                             int n0, int M, int N,
                                             const float* __restrict__ g,
                                             float* __restrict__ gp) {
  const int cn = n0 + (lane & 15);
  if (cn >= N) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cm = m0 + (lane >> 4) * 4 + i;
    if (cm >= M) continue;
    const int64_t o = (int64_t)cm * N + cn;
    gp[o] = acc[i] + g[o];
  }
}

struct CrossEpilogue {  // x_next = fmaf(x0, acc + bias, x)
  const float* bias;
  const float* x0;
  const float* x;
  float* xn;
  short* xn16;
  short* u16;
  __device__ __forceinline__ void operator()(f32x4 acc, int lane, int m0,
                                             int n0, int M, int N) const {
    cross_store(acc, lane, m0, n0, M, N, bias, x0, x, xn, xn16, u16);
  }
};

struct DxEpilogue {  // g_prev = acc + g
  const float* g;
  float* gp;
  __device__ __forceinline__ void operator()(f32x4 acc, int lane, int m0,
                                             int n0, int M, int N) const {
    dx_add_store(acc, lane, m0, n0, M, N, g, gp);
  }
};

// ------------------------------------------------------------------
// epi(A[M,K] @ W[N,K]^T). Tiling as k_linear_fwd_t<1>: 4 waves stacked on
// M, 16 rows x 64 columns each.
// ------------------------------------------------------------------
template <class Epi>
__device__ __forceinline__ void cross_gemm(const short* __restrict__ A,
                                           const short* __restrict__ W,
                                           int M, int N, int K,
                                           const Epi& epi) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ntiles64 = (N + 63) / 64;
  const int m0 = (blockIdx.x / ntiles64) * 64 + wave * 16;
  const int n0 = (blockIdx.x % ntiles64) * 64;
  if (m0 >= M) return;
  f32x4 acc[1][4] = {};
  if (m0 + 16 <= M && n0 + 64 <= N)  // wave-uniform
    fwd_accumulate<1, false>(A, W, M, N, K, m0, n0, lane, acc);
  else
    fwd_accumulate<1, true>(A, W, M, N, K, m0, n0, lane, acc);
  const int nt = min(4, (N - n0 + 15) / 16);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nt) break;
    epi(acc[0][t], lane, m0, n0 + t * 16, M, N);
  }
}

// K = N is the full-matrix layer; K = R with A = t16 is the second half of
// a low-rank layer whose first half is a plain linear_fwd without
// activation.
__global__ void __launch_bounds__(256) k_cross_fwd(
    const short* __restrict__ A, const short* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ x0,
    const float* __restrict__ x, int M, int N, int K, float* __restrict__ xn,
    short* __restrict__ xn16, short* __restrict__ u16) {
  cross_gemm(A, W, M, N, K, CrossEpilogue{bias, x0, x, xn, xn16, u16});
}

// g_prev = g + du[M,N] @ W with Wt = W^T as [N_out, N] rows.
__global__ void __launch_bounds__(256) k_cross_dx(
    const short* __restrict__ du, const short* __restrict__ Wt,
    const float* __restrict__ g, int M, int N, int K,
    float* __restrict__ gp) {
  cross_gemm(du, Wt, M, N, K, DxEpilogue{g, gp});
}

// The two element rules of the backward's elementwise step, shared by
// k_cross_du and k_cross_lr_bwd so that both layer kinds round alike.
__device__ __forceinline__ short du_elem(float g, float x0) {
  return f2bf_u16(g * x0);
}
__device__ __forceinline__ float dx0_elem(float g, short u, float dx0) {
  return fmaf(g, bf2f_u16(u), dx0);
}

// Both rules over 8 contiguous elements at p (all inside the operands).
__device__ __forceinline__ bf16x8 du_vec8(const float* __restrict__ g,
                                          const float* __restrict__ x0,
                                          const short* __restrict__ u16,
                                          float* dx0, int64_t p) {
  const f32x4 g0 = *reinterpret_cast<const f32x4_u*>(g + p);
  const f32x4 g1 = *reinterpret_cast<const f32x4_u*>(g + p + 4);
  const f32x4 y0 = *reinterpret_cast<const f32x4_u*>(x0 + p);
  const f32x4 y1 = *reinterpret_cast<const f32x4_u*>(x0 + p + 4);
  const bf16x8 u = *reinterpret_cast<const bf16x8_u*>(u16 + p);
  f32x4 d0 = *reinterpret_cast<const f32x4_u*>(dx0 + p);
  f32x4 d1 = *reinterpret_cast<const f32x4_u*>(dx0 + p + 4);
  bf16x8 du;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    du[i] = du_elem(g0[i], y0[i]);
    du[4 + i] = du_elem(g1[i], y1[i]);
    d0[i] = dx0_elem(g0[i], u[i], d0[i]);
    d1[i] = dx0_elem(g1[i], u[4 + i], d1[i]);
  }
  *reinterpret_cast<f32x4_u*>(dx0 + p) = d0;
  *reinterpret_cast<f32x4_u*>(dx0 + p + 4) = d1;
  return du;
}

// ------------------------------------------------------------------
// du16 = bf(g * x0), dx0 += g * float(u16) over n elements, 8 per thread
// and step (16-B accesses), scalar tail. Grid-stride.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cross_du(
    const float* __restrict__ g, const float* __restrict__ x0,
    const short* __restrict__ u16, float* dx0, short* __restrict__ du16,
    int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n8 = n / 8;
  for (int64_t v = tid; v < n8; v += nthreads)
    *reinterpret_cast<bf16x8_u*>(du16 + v * 8) =
        du_vec8(g, x0, u16, dx0, v * 8);
  for (int64_t p = n8 * 8 + tid; p < n; p += nthreads) {
    du16[p] = du_elem(g[p], x0[p]);
    dx0[p] = dx0_elem(g[p], u16[p], dx0[p]);
  }
}

// ------------------------------------------------------------------
// One-launch low-rank backward. A wave owns 16 rows and works alone: phase
// 1 leaves its 16 x R intermediate dt, rounded to bf16, in the wave's own
// LDS tile; phase 2 reads the tile back as A fragments, keeps them in
// registers (R <= 128 is 16 VGPRs) and sweeps the D output columns in
// chunks of 64 with the rows of the second weight as B fragments from L2.
// NT = 16-column subtiles of the intermediate (2, 4 or 8, the smallest
// with 16 * NT >= R): tile columns [R, 16 * NT) hold the zeros of phase
// 1's zero-filled B rows, so phase 2 has no K tail on the A side. Nothing
// crosses waves: a wave-level fence, no block barrier.
// ------------------------------------------------------------------
constexpr int LR_WAVES = 2;  // 32 rows per block: B = 8192 gives 256 blocks

template <int NT>
struct LrTile {  // pitch 32 * NT + 16 bytes: 16-B fragment reads of the 16
  alignas(16) short v[16][NT * 16 + 8];  // rows start in different banks
};

// Orders one wave's LDS writes against its own later reads across lanes.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Round the phase-1 accumulators into the tile, store them to t16 [M, R]
// and return the tile as phase 2's A fragments.
template <int NT>
__device__ __forceinline__ void lr_stage(const f32x4 (&acc)[NT],
                                         LrTile<NT>& tile, int lane, int m0,
                                         int M, int R,
                                         short* __restrict__ t16,
                                         bf16x8 (&tf)[NT / 2]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int cn = t * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (lane >> 4) * 4 + i;
      const short v = f2bf_u16(acc[t][i]);
      tile.v[r][cn] = v;
      if (cn < R && m0 + r < M) t16[(int64_t)(m0 + r) * R + cn] = v;
    }
  }
  wave_lds_fence();
#pragma unroll
  for (int s = 0; s < NT / 2; ++s)
    tf[s] = *reinterpret_cast<const bf16x8*>(
        &tile.v[lane & 15][s * 32 + (lane >> 4) * 8]);
}

// acc = tf[16, R] @ W[N, R]^T for the 64 columns at n0: the MFMAs of
// fwd_accumulate<1>(t16, W, M, N, R, ...) in the same ascending-k order.
// B fragments outside W are zeros (never products: the A side holds zeros
// there, but W's neighbourhood may hold NaN).
template <int NT>
__device__ __forceinline__ void lr_chunk(const bf16x8 (&tf)[NT / 2],
                                         const short* __restrict__ W, int N,
                                         int R, int n0, int lane,
                                         f32x4 (&acc)[4]) {
  const int kgrp = (lane >> 4) * 8;
  const int ksteps = (R + 31) / 32;
  const bool direct = n0 + 64 <= N && (R & 7) == 0;  // wave-uniform
  const bf16x8 zero = {};
#pragma unroll
  for (int s = 0; s < NT / 2; ++s) {
    if (s >= ksteps) break;
    const int k = s * 32 + kgrp;
    bf16x8 b[4];
    if (direct) {  // a lane's fragment is wholly inside or outside R
      const bool kin = k < R;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        b[t] = *reinterpret_cast<const bf16x8_u*>(
            W + (int64_t)(n0 + t * 16 + (lane & 15)) * R + (kin ? k : 0));
#pragma unroll
      for (int t = 0; t < 4; ++t) b[t] = kin ? b[t] : zero;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        b[t] = load_frag_row(W, n0 + t * 16 + (lane & 15), k, N, R);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf[s], b[t], acc[t],
                                                       0, 0, 0);
  }
}

// Phase 2: epi over every 64-column chunk of N.
template <int NT, class Epi>
__device__ __forceinline__ void lr_sweep(const bf16x8 (&tf)[NT / 2],
                                         const short* __restrict__ W, int M,
                                         int N, int R, int m0, int lane,
                                         const Epi& epi) {
  for (int n0 = 0; n0 < N; n0 += 64) {
    f32x4 acc[4] = {};
    lr_chunk<NT>(tf, W, N, R, n0, lane, acc);
    const int nt = min(4, (N - n0 + 15) / 16);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= nt) break;
      epi(acc[t], lane, m0, n0 + t * 16, M, N);
    }
  }
}

// Data gradient of the low-rank layer: g [M, D], x0, dx0 fp32, u16 = bf(u)
// saved by the forward, Ut = bf(U)^T [R, D], Vt = bf(V)^T [D, R].
// Phase 1 sweeps D in 32-wide K steps: each lane forms its 8 elements of
// du = bf(g * x0) in registers (the A fragment: row lane%16, k 8*(lane/16)
// + i), stores them to du16, updates its 8 elements of dx0 in place and
// feeds NT MFMAs against the rows of Ut. Every (row, k) belongs to exactly
// one lane of one wave, so the in-place update needs no atomics.
template <int NT>
__global__ void __launch_bounds__(64 * LR_WAVES) k_cross_lr_bwd(
    const float* __restrict__ g, const float* __restrict__ x0,
    const short* __restrict__ u16, const short* __restrict__ Ut,
    const short* __restrict__ Vt, int M, int D, int R, float* dx0,
    float* __restrict__ gp, short* __restrict__ du16,
    short* __restrict__ dt16) {
  __shared__ LrTile<NT> tiles[LR_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m0 = (blockIdx.x * LR_WAVES + wave) * 16;
  if (m0 >= M) return;
  const int kgrp = (lane >> 4) * 8;
  const int row = m0 + (lane & 15);
  const bool row_ok = row < M;
  const bf16x8 zero = {};
  // this lane's B rows of Ut, clamped into the operand
  const short* bp[NT];
  bool b_ok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = t * 16 + (lane & 15);
    b_ok[t] = n < R;
    bp[t] = Ut + (int64_t)min(n, R - 1) * D + kgrp;
  }
  f32x4 acc[NT] = {};
  for (int k0 = 0; k0 < D; k0 += 32) {
    const int k = k0 + kgrp;
    const int64_t p = (int64_t)row * D + k;
    bf16x8 b[NT];
    bf16x8 du = zero;
    if (k0 + 32 <= D) {  // wave-uniform: every fragment is inside D
#pragma unroll
      for (int t = 0; t < NT; ++t)
        b[t] = *reinterpret_cast<const bf16x8_u*>(bp[t] + k0);
      if (row_ok) {
        du = du_vec8(g, x0, u16, dx0, p);
        *reinterpret_cast<bf16x8_u*>(du16 + p) = du;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t] = b_ok[t] ? b[t] : zero;
    } else {  // the K tail, element by element
#pragma unroll
      for (int t = 0; t < NT; ++t)
        b[t] = load_frag_row(Ut, t * 16 + (lane & 15), k, R, D);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!row_ok || k + i >= D) continue;
        du[i] = du_elem(g[p + i], x0[p + i]);
        dx0[p + i] = dx0_elem(g[p + i], u16[p + i], dx0[p + i]);
        du16[p + i] = du[i];
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(du, b[t], acc[t], 0,
                                                       0, 0);
  }
  bf16x8 tf[NT / 2];
  lr_stage<NT>(acc, tiles[wave], lane, m0, M, R, dt16, tf);
  lr_sweep<NT>(tf, Vt, M, D, R, m0, lane, DxEpilogue{g, gp});
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

static void check_shape(const torch::Tensor& t, int64_t rows, int64_t cols,
                        const char* op, const char* name) {
  TORCH_CHECK(t.size(0) == rows && t.size(1) == cols, op, ": ", name,
              " is [", t.size(0), ",", t.size(1), "], expected [", rows, ",",
              cols, "]");
}

// a [B, D] matrix of the given dtype
static void check_operand(const torch::Tensor& t, c10::ScalarType dtype,
                          int64_t B, int64_t D, const char* op,
                          const char* name) {
  check_matrix(t, dtype, op, name);
  check_shape(t, B, D, op, name);
}

static void check_extent(const char* op, int64_t B, int64_t D) {
  TORCH_CHECK(B * D < (1LL << 31) && B < (1 << 30), op,
              ": B and B*D must stay below 2^31");
}

static void check_one_device(
    const char* op, std::initializer_list<const torch::Tensor*> ts) {
  const auto dev = (*ts.begin())->device();
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->device() == dev, op,
                ": all operands must be on one device, got ", t->device(),
                " and ", dev);
}

// bias [D] fp32 and the fp32 residual operands x0, x [B, D] of a forward
static void check_cross_operands(const char* op, const torch::Tensor& bias,
                                 const torch::Tensor& x0,
                                 const torch::Tensor& x, int64_t B,
                                 int64_t D) {
  TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == torch::kFloat32 &&
                  bias.dim() == 1 && bias.numel() == D &&
                  bias.is_contiguous(),
              op, ": bias must be a contiguous fp32 GPU vector of ", D);
  check_operand(x0, torch::kFloat32, B, D, op, "x0");
  check_operand(x, torch::kFloat32, B, D, op, "x");
  check_extent(op, B, D);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> cross_fwd(
    torch::Tensor a16, torch::Tensor w16, torch::Tensor bias,
    torch::Tensor x0, torch::Tensor x, bool save_u) {
  const char* op = "cross_fwd";
  check_matrix(a16, torch::kBFloat16, op, "a16");
  check_matrix(w16, torch::kBFloat16, op, "w16");
  TORCH_CHECK(a16.size(1) == w16.size(1), op, ": a16 is [B,", a16.size(1),
              "] but w16 is [D,", w16.size(1), "]");
  const int64_t B = a16.size(0), K = a16.size(1), D = w16.size(0);
  TORCH_CHECK(K >= 1 && D >= 1, op, ": empty weight");
  check_cross_operands(op, bias, x0, x, B, D);
  check_one_device(op, {&a16, &w16, &bias, &x0, &x});
  auto xn = torch::empty_like(x);
  auto xn16 = torch::empty({B, D}, a16.options());
  auto u16 = torch::empty({save_u ? B : 0, D}, a16.options());
  if (B == 0) return {xn, xn16, u16};
  const int blocks = (int)(((B + 63) / 64) * ((D + 63) / 64));
  k_cross_fwd<<<blocks, 256, 0, current_hip_stream()>>>(
      bf_ptr(a16), bf_ptr(w16), bias.data_ptr<float>(),
      x0.data_ptr<float>(), x.data_ptr<float>(), (int)B, (int)D, (int)K,
      xn.data_ptr<float>(), bf_ptr_mut(xn16),
      save_u ? bf_ptr_mut(u16) : nullptr);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {xn, xn16, u16};
}

// du16 = bf(g * x0); dx0 += g * float(u16) in place.
torch::Tensor cross_du(torch::Tensor g, torch::Tensor x0, torch::Tensor u16,
                       torch::Tensor dx0) {
  const char* op = "cross_du";
  check_matrix(g, torch::kFloat32, op, "g");
  const int64_t B = g.size(0), D = g.size(1);
  check_operand(x0, torch::kFloat32, B, D, op, "x0");
  check_operand(u16, torch::kBFloat16, B, D, op, "u16");
  check_operand(dx0, torch::kFloat32, B, D, op, "dx0");
  check_extent(op, B, D);
  check_one_device(op, {&g, &x0, &u16, &dx0});
  auto du16 = torch::empty_like(u16);
  const int64_t n = B * D;
  if (n == 0) return du16;
  k_cross_du<<<n_blocks((n + 7) / 8), 256, 0, current_hip_stream()>>>(
      g.data_ptr<float>(), x0.data_ptr<float>(), bf_ptr(u16),
      dx0.data_ptr<float>(), bf_ptr_mut(du16), n);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return du16;
}

// g_prev = g + du16 @ W, with wt16 = bf(W)^T contiguous.
torch::Tensor cross_dx(torch::Tensor du16, torch::Tensor wt16,
                       torch::Tensor g) {
  const char* op = "cross_dx";
  check_matrix(du16, torch::kBFloat16, op, "du16");
  check_matrix(wt16, torch::kBFloat16, op, "wt16");
  const int64_t B = du16.size(0), K = du16.size(1), D = wt16.size(0);
  TORCH_CHECK(wt16.size(1) == K, op, ": du16 is [B,", K, "] but wt16 is [D,",
              wt16.size(1), "]");
  TORCH_CHECK(K >= 1 && D >= 1, op, ": empty weight");
  check_operand(g, torch::kFloat32, B, D, op, "g");
  check_extent(op, B, std::max(D, K));
  check_one_device(op, {&du16, &wt16, &g});
  auto gp = torch::empty_like(g);
  if (B == 0) return gp;
  const int blocks = (int)(((B + 63) / 64) * ((D + 63) / 64));
  k_cross_dx<<<blocks, 256, 0, current_hip_stream()>>>(
      bf_ptr(du16), bf_ptr(wt16), g.data_ptr<float>(), (int)B, (int)D,
      (int)K, gp.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return gp;
}

static void check_rank(const char* op, int64_t R) {
  TORCH_CHECK(R >= 1 && R <= 128, op, ": the rank must be in [1, 128], got ",
              R);
}

// launch KERNEL<NT> with the smallest NT in {2, 4, 8} that covers R
#define LR_DISPATCH(R, KERNEL, blocks, ...)                                 \
  do {                                                                      \
    if ((R) <= 32)                                                          \
      KERNEL<2><<<blocks, 64 * LR_WAVES, 0, current_hip_stream()>>>(        \
          __VA_ARGS__);                                                     \
    else if ((R) <= 64)                                                     \
      KERNEL<4><<<blocks, 64 * LR_WAVES, 0, current_hip_stream()>>>(        \
          __VA_ARGS__);                                                     \
    else                                                                    \
      KERNEL<8><<<blocks, 64 * LR_WAVES, 0, current_hip_stream()>>>(        \
          __VA_ARGS__);                                                     \
  } while (0)

static int lr_blocks(int64_t B) {
  return (int)((B + 16 * LR_WAVES - 1) / (16 * LR_WAVES));
}

// ut16 = bf(U)^T [R, D], vt16 = bf(V)^T [D, R]; dx0 is updated in place.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> cross_lr_bwd(
    torch::Tensor g, torch::Tensor x0, torch::Tensor u16, torch::Tensor ut16,
    torch::Tensor vt16, torch::Tensor dx0) {
  const char* op = "cross_lr_bwd";
  check_matrix(g, torch::kFloat32, op, "g");
  check_matrix(ut16, torch::kBFloat16, op, "ut16");
  const int64_t B = g.size(0), D = g.size(1), R = ut16.size(0);
  check_rank(op, R);
  TORCH_CHECK(D >= 1, op, ": empty weight");
  check_operand(ut16, torch::kBFloat16, R, D, op, "ut16");
  check_operand(vt16, torch::kBFloat16, D, R, op, "vt16");
  check_operand(x0, torch::kFloat32, B, D, op, "x0");
  check_operand(u16, torch::kBFloat16, B, D, op, "u16");
  check_operand(dx0, torch::kFloat32, B, D, op, "dx0");
  check_extent(op, B, D);
  check_one_device(op, {&g, &x0, &u16, &ut16, &vt16, &dx0});
  auto gp = torch::empty_like(g);
  auto du16 = torch::empty_like(u16);
  auto dt16 = torch::empty({B, R}, u16.options());
  if (B == 0) return {gp, du16, dt16};
  LR_DISPATCH(R, k_cross_lr_bwd, lr_blocks(B), g.data_ptr<float>(),
              x0.data_ptr<float>(), bf_ptr(u16), bf_ptr(ut16), bf_ptr(vt16),
              (int)B, (int)D, (int)R, dx0.data_ptr<float>(),
              gp.data_ptr<float>(), bf_ptr_mut(du16), bf_ptr_mut(dt16));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {gp, du16, dt16};
}

void register_cross(py::module_& mod) {
  mod.def("cross_fwd", &cross_fwd, py::arg("a16"), py::arg("w16"),
          py::arg("bias"), py::arg("x0"), py::arg("x"), py::arg("save_u"));
  mod.def("cross_du", &cross_du, py::arg("g"), py::arg("x0"),
          py::arg("u16"), py::arg("dx0"));
  mod.def("cross_dx", &cross_dx, py::arg("du16"), py::arg("wt16"),
          py::arg("g"));
  mod.def("cross_lr_bwd", &cross_lr_bwd, py::arg("g"), py::arg("x0"),
          py::arg("u16"), py::arg("ut16"), py::arg("vt16"), py::arg("dx0"));
}
