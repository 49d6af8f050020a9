// loss_kernels.hip — fused binary cross-entropy with logits (mean) for the
// end of the captured training step.
//
// torch's binary_cross_entropy_with_logits + autograd is 6 elementwise /
// reduce launches forward and 5 backward for a few tens of KB. Here it is
// one launch each way.
//
// Forward: l_i = max(x,0) - x*y + log1p(exp(-|x|)); loss = sum(l_i) / B.
// The sum has a fixed shape, so the result does not depend on scheduling:
// thread t adds elements t, t+kLossBlock, ... in order, then the block
// folds its kLossBlock partials in a binary LDS tree. One block, no atomics.
//
// Backward: g_i = (sigmoid(x) - y) * grad_out / B, with sigmoid(x) - y
// evaluated over the common denominator 1 + e, e = exp(-|x|):
//   x >= 0: ((1 - y) - y*e) / (1 + e)      x < 0: (e*(1 - y) - y) / (1 + e)
// so the cancellation of sigmoid(x) against y happens inside one fma whose
// rounding is relative to the (small) result. grad_out is read on the
// device: no host sync, capture-safe.

#include "hip_common.h"

namespace {

constexpr int kLossBlock = 1024;
// Single-block cap of the forward kernel: above it the per-thread serial
// chain (B / kLossBlock adds) stops being short and the Python wrapper falls
// back to torch.
constexpr int64_t kLossMaxB = 1 << 20;

__global__ __launch_bounds__(kLossBlock) void k_bce_logits_mean_fwd(
    const float* __restrict__ x, const float* __restrict__ y, int n,
    float* __restrict__ loss) {
  __shared__ float part[kLossBlock];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < n; i += kLossBlock) {
    const float xi = x[i];
    acc += (fmaxf(xi, 0.0f) - xi * y[i]) + log1pf(expf(-fabsf(xi)));
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kLossBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] / (float)n;
}

__global__ void k_bce_logits_mean_bwd(const float* __restrict__ x,
                                      const float* __restrict__ y,
                                      const float* __restrict__ grad_out,
                                      int n, float* __restrict__ gx) {
  const float scale = grad_out[0] / (float)n;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int stride = gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const float xi = x[i], yi = y[i];
    const float e = expf(-fabsf(xi));
    const float omy = 1.0f - yi;
    const float num = xi >= 0.0f ? fmaf(-yi, e, omy) : fmaf(e, omy, -yi);
    gx[i] = (num / (1.0f + e)) * scale;
  }
}

void check_loss_inputs(const torch::Tensor& logits,
                       const torch::Tensor& labels) {
  TORCH_CHECK(logits.is_cuda() && labels.is_cuda(),
              "bce_logits_mean: inputs must be on GPU");
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32 &&
                  labels.scalar_type() == torch::kFloat32,
              "bce_logits_mean: inputs must be fp32");
  TORCH_CHECK(logits.dim() == 1 && labels.dim() == 1 &&
                  logits.numel() == labels.numel(),
              "bce_logits_mean: logits and labels must be [B]");
  TORCH_CHECK(logits.is_contiguous() && labels.is_contiguous(),
              "bce_logits_mean: inputs must be contiguous");
  TORCH_CHECK(logits.numel() >= 1 && logits.numel() <= kLossMaxB,
              "bce_logits_mean: B must be in [1, ", kLossMaxB, "]");
}

}  // namespace

torch::Tensor bce_logits_mean_fwd(torch::Tensor logits,
                                  torch::Tensor labels) {
  check_loss_inputs(logits, labels);
  auto loss = torch::empty({}, logits.options());
  k_bce_logits_mean_fwd<<<1, kLossBlock, 0, current_hip_stream()>>>(
      logits.data_ptr<float>(), labels.data_ptr<float>(),
      (int)logits.numel(), loss.data_ptr<float>());
  return loss;
}

torch::Tensor bce_logits_mean_bwd(torch::Tensor logits, torch::Tensor labels,
                                  torch::Tensor grad_out) {
  check_loss_inputs(logits, labels);
  TORCH_CHECK(grad_out.is_cuda() && grad_out.numel() == 1 &&
                  grad_out.scalar_type() == torch::kFloat32,
              "bce_logits_mean: grad_out must be one fp32 value on GPU");
  auto gx = torch::empty_like(logits);
  const int n = (int)logits.numel();
  k_bce_logits_mean_bwd<<<n_blocks(n), 256, 0, current_hip_stream()>>>(
      logits.data_ptr<float>(), labels.data_ptr<float>(),
      grad_out.data_ptr<float>(), n, gx.data_ptr<float>());
  return gx;
}

void register_loss(py::module_& mod) {
  mod.def("bce_logits_mean_fwd", &bce_logits_mean_fwd);
  mod.def("bce_logits_mean_bwd", &bce_logits_mean_bwd);
  // largest B the single-block forward takes; larger batches use torch
  mod.attr("BCE_LOGITS_MEAN_MAX_B") = kLossMaxB;
}
