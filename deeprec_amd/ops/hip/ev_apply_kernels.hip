// ev_apply_kernels.hip — the embedding write surface for gfx950: the fused
// sparse optimizer applies on slot indices (no second probe), ONE kernel
// body instantiated per update rule, and ONE host launcher that checks what
// the kernel takes on trust.
//
// A rule is a small struct passed to the kernel by value: w, the rule's
// state slabs, its hyperparameters; operator()(o, slot, g) updates element
// o of w and of the slabs with gradient g. Shared by the rules:
// second_moment(), adam_step() and adagrad_step(). Thread mapping: thread =
// (unique key i, dim element d), grid-stride (see n_blocks in hip_common.h).

#include "hip_common.h"

#include <initializer_list>
#include <limits>

namespace py = pybind11;
using torch::Tensor;

#define DEV_INLINE __device__ __forceinline__

namespace {

constexpr int kBlock = 256;

// vel[o] <- beta2 * vel[o] + (1 - beta2) * g^2; returns the new value
DEV_INLINE float second_moment(float* __restrict__ vel, int64_t o,
                               float beta2, float g) {
  const float vn = beta2 * vel[o] + (1.0f - beta2) * g * g;
  vel[o] = vn;
  return vn;
}

// Updates both Adam moments at o; returns what w[o] moves by.
DEV_INLINE float adam_step(float* __restrict__ mom, float* __restrict__ vel,
                           int64_t o, float g, float lr_t, float beta1,
                           float beta2, float epsilon) {
  const float mn = beta1 * mom[o] + (1.0f - beta1) * g;
  const float vn = second_moment(vel, o, beta2, g);
  mom[o] = mn;
  return lr_t * mn / (sqrtf(vn) + epsilon);
}

// a: the accumulator after this gradient
DEV_INLINE void adagrad_step(float* __restrict__ w, int64_t o, float g,
                             float a, float lr, float epsilon) {
  w[o] -= lr * g / (sqrtf(a) + epsilon);
}

struct SgdRule {
  float* __restrict__ w;
  float lr;
  DEV_INLINE void operator()(int64_t o, int32_t, float g) const {
    w[o] -= lr * g;
  }
};

struct AdagradRule {
  float *__restrict__ w, *__restrict__ accum;
  float lr, epsilon;
  DEV_INLINE void operator()(int64_t o, int32_t, float g) const {
    const float a = accum[o] + g * g;
    accum[o] = a;
    adagrad_step(w, o, g, a, lr, epsilon);
  }
};

// Periodic accumulator decay; period bookkeeping is per-slot (1-wide slab).
struct AdagradDecayRule {
  float *__restrict__ w, *__restrict__ accum;
  const float* __restrict__ period_slab;
  float lr, epsilon, cur_period, decay_rate, baseline;
  DEV_INLINE void operator()(int64_t o, int32_t slot, float g) const {
    const float prev_period = period_slab[slot];
    float dp = cur_period - prev_period;
    if (dp < 0.0f) dp = 0.0f;
    const float decay = powf(decay_rate, dp);
    float a = accum[o] * decay;
    if (a < baseline) a = baseline;
    a += g * g;
    accum[o] = a;
    adagrad_step(w, o, g, a, lr, epsilon);
    // period_slab is committed by a separate k_commit_period launch so every
    // (key, d) thread here reads the pre-update period value.
  }
};

struct AdamRule {
  float *__restrict__ w, *__restrict__ mom, *__restrict__ vel;
  float lr_t, beta1, beta2, epsilon;
  DEV_INLINE void operator()(int64_t o, int32_t, float g) const {
    w[o] -= adam_step(mom, vel, o, g, lr_t, beta1, beta2, epsilon);
  }
};

// AdamRule whose bias correction comes from powers = [beta1^t, beta2^t] on
// the device (k_update_powers), for captured steps: see prepared().
struct AdamDevRule {
  float *__restrict__ w, *__restrict__ mom, *__restrict__ vel;
  float lr, beta1, beta2, epsilon;
  const float* __restrict__ powers;
};

struct AdamWRule {
  float *__restrict__ w, *__restrict__ mom, *__restrict__ vel;
  float lr_t, lr, beta1, beta2, epsilon, weight_decay;
  DEV_INLINE void operator()(int64_t o, int32_t, float g) const {
    const float step = adam_step(mom, vel, o, g, lr_t, beta1, beta2, epsilon);
    const float wv = w[o];
    w[o] = wv - step - lr * weight_decay * wv;
  }
};

struct RmspropRule {
  float *__restrict__ w, *__restrict__ vel;
  float lr, beta2, epsilon;
  DEV_INLINE void operator()(int64_t o, int32_t, float g) const {
    const float vn = second_moment(vel, o, beta2, g);
    w[o] -= lr * g / (sqrtf(vn) + epsilon);
  }
};

// l2_shrinkage != 0 is the FtrlV2 variant (reference:
// KvResourceSparseApplyFtrlV2): the linear term sees
// g + 2*l2_shrinkage*w while the accumulator sees plain g^2.
struct FtrlRule {
  float *__restrict__ w, *__restrict__ n, *__restrict__ z;
  float lr, l1, l2, lr_power, l2_shrinkage;
  DEV_INLINE void operator()(int64_t o, int32_t, float g) const {
    const float wv = w[o];
    const float n_old = n[o];
    const float n_new = n_old + g * g;
    const float sigma =
        (powf(n_new, -lr_power) - powf(n_old, -lr_power)) / lr;
    const float gs = g + 2.0f * l2_shrinkage * wv;
    const float z_new = z[o] + gs - sigma * wv;
    n[o] = n_new;
    z[o] = z_new;
    const float quad = powf(n_new, -lr_power) / lr + 2.0f * l2;
    float w_new = 0.0f;
    if (fabsf(z_new) > l1)
      w_new = ((z_new > 0.0f ? l1 : -l1) - z_new) / quad;
    w[o] = w_new;
  }
};

// What a thread does once, before its loop.
template <typename Rule>
DEV_INLINE Rule prepared(const Rule& rule) {
  return rule;
}

DEV_INLINE AdamRule prepared(const AdamDevRule& r) {
  const float lr_t =
      r.lr * sqrtf(1.0f - r.powers[1]) / (1.0f - r.powers[0]);
  return {r.w, r.mom, r.vel, lr_t, r.beta1, r.beta2, r.epsilon};
}

// grad is [m, dim], row i for slots[i]; slots[i] < 0 (not admitted, or the
// padded tail of a captured step) is skipped. PRECONDITION: the slots other
// than -1 are distinct within a call (they come from a dedup) — that is
// what makes the rules' unsynchronised read-modify-write correct.
template <typename Rule>
__global__ void k_sparse_apply(const int32_t* __restrict__ slots,
                               const float* __restrict__ grad, int m, int dim,
                               Rule rule) {
  const auto apply = prepared(rule);
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)m * dim;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int i = (int)(t / dim);
    const int d = (int)(t % dim);
    const int32_t s = slots[i];
    if (s < 0) continue;
    const int64_t o = (int64_t)s * dim + d;
    apply(o, s, grad[t]);
  }
}

__global__ void k_commit_period(float* __restrict__ period_slab,
                                const int32_t* __restrict__ slots, int m,
                                float cur_period) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t gstride = gridDim.x * (int64_t)blockDim.x;
  for (; i < m; i += gstride) {
    int32_t sl = slots[i];
    if (sl >= 0) period_slab[sl] = cur_period;
  }
}

__global__ void k_update_powers(float* __restrict__ powers, float beta1,
                                float beta2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    powers[0] *= beta1;
    powers[1] *= beta2;
  }
}

}  // namespace

// ------------------------------------------------------------------
// host side
// ------------------------------------------------------------------

// The rules are built before the launcher has checked a dtype, so they take
// their pointers untyped.
static float* f32(const Tensor& t) { return static_cast<float*>(t.data_ptr()); }

static bool f32_on(const Tensor& t, const Tensor& w) {
  return t.device() == w.device() && t.scalar_type() == torch::kFloat32 &&
         t.is_contiguous();
}

// A state slab of w: one row per row of w, `width` wide.
static bool slab_of(const Tensor& t, const Tensor& w, int64_t width) {
  return f32_on(t, w) && t.dim() == 2 && t.size(0) == w.size(0) &&
         t.size(1) == width;
}

// Everything k_sparse_apply<Rule> takes on trust is checked here, on the
// host and without a sync (safe under capture); then the one launch.
// `slabs` are the rule's state slabs of w's shape. Returns false when there
// is nothing to apply.
template <typename Rule>
static bool launch_apply(const char* name, const Tensor& w,
                         std::initializer_list<Tensor> slabs,
                         const Tensor& slots, const Tensor& grad, Rule rule) {
  const int64_t m = slots.numel();
  if (m == 0) return false;
  TORCH_CHECK(w.is_cuda() && f32_on(w, w) && w.dim() == 2 && w.size(1) > 0,
              name, ": w must be a contiguous fp32 [slots, dim] on GPU");
  const int64_t dim = w.size(1);
  TORCH_CHECK(slots.device() == w.device() &&
                  slots.scalar_type() == torch::kInt32 && slots.dim() == 1 &&
                  slots.is_contiguous(),
              name, ": slots must be a contiguous int32 [m] on w's device");
  TORCH_CHECK(f32_on(grad, w) && grad.numel() == m * dim, name,
              ": grad must be a contiguous fp32 [m, dim] on w's device");
  for (const Tensor& s : slabs)
    TORCH_CHECK(slab_of(s, w, dim), name,
                ": a state slab must be a contiguous fp32 of w's shape on "
                "w's device, got ", s.sizes());
  // the kernel takes m and dim as int (their product as int64)
  TORCH_CHECK(m <= std::numeric_limits<int>::max() &&
                  dim <= std::numeric_limits<int>::max(),
              name, ": m and dim must fit an int");
  k_sparse_apply<Rule>
      <<<n_blocks(m * dim), kBlock, 0, current_hip_stream()>>>(
          static_cast<const int32_t*>(slots.data_ptr()), f32(grad), (int)m,
          (int)dim, rule);
  return true;
}

// powers = [beta1^t, beta2^t], advanced on the device by update_powers
static void check_powers(const Tensor& powers) {
  TORCH_CHECK(powers.is_cuda() && powers.scalar_type() == torch::kFloat32 &&
                  powers.is_contiguous() && powers.numel() >= 2,
              "powers must be fp32 [2] on GPU");
}

void apply_sgd(Tensor w, Tensor slots, Tensor grad, float lr) {
  launch_apply("apply_sgd", w, {}, slots, grad, SgdRule{f32(w), lr});
}

void apply_adagrad(Tensor w, Tensor accum, Tensor slots, Tensor grad,
                   float lr, float epsilon) {
  launch_apply("apply_adagrad", w, {accum}, slots, grad,
               AdagradRule{f32(w), f32(accum), lr, epsilon});
}

void apply_adagrad_decay(Tensor w, Tensor accum, Tensor period_slab,
                         Tensor slots, Tensor grad, float lr, float epsilon,
                         float cur_period, float decay_rate, float baseline) {
  TORCH_CHECK(w.dim() == 2 && slab_of(period_slab, w, 1),
              "apply_adagrad_decay: the period slab must be a contiguous "
              "fp32 [slots, 1] on w's device");
  if (!launch_apply("apply_adagrad_decay", w, {accum}, slots, grad,
                    AdagradDecayRule{f32(w), f32(accum), f32(period_slab), lr,
                                     epsilon, cur_period, decay_rate,
                                     baseline}))
    return;
  const int m = (int)slots.numel();
  k_commit_period<<<n_blocks(m), kBlock, 0, current_hip_stream()>>>(
      f32(period_slab), slots.data_ptr<int32_t>(), m, cur_period);
}

void apply_adam(Tensor w, Tensor mom, Tensor vel, Tensor slots, Tensor grad,
                float lr_t, float beta1, float beta2, float epsilon) {
  launch_apply("apply_adam", w, {mom, vel}, slots, grad,
               AdamRule{f32(w), f32(mom), f32(vel), lr_t, beta1, beta2,
                        epsilon});
}

void apply_adam_dev(Tensor w, Tensor mom, Tensor vel, Tensor slots,
                    Tensor grad, float lr, float beta1, float beta2,
                    float epsilon, Tensor powers) {
  check_powers(powers);
  launch_apply("apply_adam_dev", w, {mom, vel}, slots, grad,
               AdamDevRule{f32(w), f32(mom), f32(vel), lr, beta1, beta2,
                           epsilon, f32(powers)});
}

void update_powers(Tensor powers, float beta1, float beta2) {
  check_powers(powers);
  k_update_powers<<<1, 64, 0, current_hip_stream()>>>(f32(powers), beta1,
                                                      beta2);
}

void apply_adamw(Tensor w, Tensor mom, Tensor vel, Tensor slots, Tensor grad,
                 float lr_t, float lr, float beta1, float beta2,
                 float epsilon, float weight_decay) {
  launch_apply("apply_adamw", w, {mom, vel}, slots, grad,
               AdamWRule{f32(w), f32(mom), f32(vel), lr_t, lr, beta1, beta2,
                         epsilon, weight_decay});
}

void apply_rmsprop(Tensor w, Tensor vel, Tensor slots, Tensor grad, float lr,
                   float beta2, float epsilon) {
  launch_apply("apply_rmsprop", w, {vel}, slots, grad,
               RmspropRule{f32(w), f32(vel), lr, beta2, epsilon});
}

void apply_ftrl(Tensor w, Tensor n, Tensor z, Tensor slots, Tensor grad,
                float lr, float l1, float l2, float lr_power,
                float l2_shrinkage) {
  launch_apply("apply_ftrl", w, {n, z}, slots, grad,
               FtrlRule{f32(w), f32(n), f32(z), lr, l1, l2, lr_power,
                        l2_shrinkage});
}

void register_ev_apply(py::module_& mod) {
  mod.def("apply_sgd", &apply_sgd);
  mod.def("apply_adagrad", &apply_adagrad);
  mod.def("apply_adagrad_decay", &apply_adagrad_decay);
  mod.def("apply_adam", &apply_adam);
  mod.def("apply_adamw", &apply_adamw);
  mod.def("apply_adam_dev", &apply_adam_dev);
  mod.def("update_powers", &update_powers);
  mod.def("apply_rmsprop", &apply_rmsprop);
  mod.def("apply_ftrl", &apply_ftrl);
}
