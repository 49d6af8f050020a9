// cross_kernels.hip — DCNv2 cross layers for gfx950 (CDNA4 MFMA).
//
// A cross layer is x_{l+1} = x0 * u_l + x_l with u_l = W_l x_l + b_l, or,
// low rank, u_l = U_l (V_l x_l) + b_l. The residual stream x stays fp32;
// the GEMM operands are bf16 (docs/KERNELS.md, "Cross layers", has the
// whole numerical contract):
//   a_l = bf(x_l)
//   u_l = a_l · bf(W_l)^T + b_l                    fp32 MFMA accumulation
//   t_l = bf(a_l · bf(V_l)^T), u_l = t_l · bf(U_l)^T + b_l     (low rank)
//   x_{l+1} = fmaf(x0, u_l, x_l)                   one rounding
// The kernel emits x_{l+1}, a_{l+1} = bf(x_{l+1}) for the next layer's
// GEMM, and on request bf(u_l).
//
//   k_cross_fwd  a GEMM with the cross epilogue; the operand side is the
//                linear forward's K loop (mfma_fwd.h)
// This file holds the forward of the full-matrix layer (and of the second
// half of a low-rank one); there is no fused backward.

#include "hip_common.h"
#include "mfma_fwd.h"

namespace py = pybind11;

namespace {

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

// ------------------------------------------------------------------
// x_next = fmaf(x0, A[M,K] @ W[N,K]^T + bias, x). Tiling as k_linear_fwd_t
// <1>: 4 waves stacked on M, 16 rows x 64 columns each. K = N is the full-
// matrix layer; K = R with A = t16 is the second half of a low-rank layer
// whose first half is a plain linear_fwd without activation.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cross_fwd(
    const short* __restrict__ A, const short* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ x0,
    const float* __restrict__ x, int M, int N, int K, float* __restrict__ xn,
    short* __restrict__ xn16, short* __restrict__ u16) {
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
    cross_store(acc[0][t], lane, m0, n0 + t * 16, M, N, bias, x0, x, xn,
                xn16, u16);
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

static void check_shape(const torch::Tensor& t, int64_t rows, int64_t cols,
                        const char* op, const char* name) {
  TORCH_CHECK(t.size(0) == rows && t.size(1) == cols, op, ": ", name,
              " is [", t.size(0), ",", t.size(1), "], expected [", rows, ",",
              cols, "]");
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
  check_matrix(x0, torch::kFloat32, op, "x0");
  check_matrix(x, torch::kFloat32, op, "x");
  check_shape(x0, B, D, op, "x0");
  check_shape(x, B, D, op, "x");
  TORCH_CHECK(B * D < (1LL << 31) && B < (1 << 30), op,
              ": B and B*D must stay below 2^31");
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
  for (const torch::Tensor* t : {&w16, &bias, &x0, &x})
    TORCH_CHECK(t->device() == a16.device(), op,
                ": all operands must be on one device, got ", t->device(),
                " and ", a16.device());
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

void register_cross(py::module_& mod) {
  mod.def("cross_fwd", &cross_fwd, py::arg("a16"), py::arg("w16"),
          py::arg("bias"), py::arg("x0"), py::arg("x"), py::arg("save_u"));
}
