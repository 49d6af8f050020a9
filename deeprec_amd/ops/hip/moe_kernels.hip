// moe_kernels.hip — grouped experts and the gate mixture of MMoE / PLE for
// gfx950 (CDNA4 MFMA). docs/KERNELS.md ("moe_kernels.hip") has the whole
// numerical contract.
//
// E experts of identical layer shapes are E small GEMMs; one launch runs
// them all. Every stacked operand is expert-major and contiguous:
// activations and gradients [E, B, .], weights [E, N, K], the mixture
// [T, B, H], so that an expert's slab is a plain row-major matrix and the
// per-slab result equals what the per-layer kernels of dense_kernels.hip
// give, bit for bit (same K loop, mfma_fwd.h; same element rules,
// mfma_epilogue.h).
//
//   k_expert_fwd      act(a_e @ w_e^T + b_e), the expert as grid z
//   k_expert_mix_fwd  the last expert layer and the gate mixture: a wave
//                     keeps its 16 x 64 tile of mix[t] in registers across
//                     the expert loop; the [B, E, H] fp32 stack, its
//                     softmax and the einsum never reach memory
//   k_expert_mix_bwd  one wave per sample: dL/d(expert outputs) and
//                     dL/d(gate logits), shuffle reductions, no atomics
//   k_expert_dx       g_e @ w_e per expert, or summed over the experts in
//                     one accumulator (the shared input's gradient)
//
// Which experts a task mixes is structure, not data: the [T, E] mask is a
// host tensor, packed into one bit set per task and passed by value, so a
// masked expert is a scalar branch and is skipped, never multiplied by 0.

#include "hip_common.h"
#include "mfma_fwd.h"
#include "mfma_epilogue.h"

namespace py = pybind11;

namespace {

constexpr int MOE_MAX_E = 16;
constexpr int MOE_MAX_T = 4;
static_assert(MOE_MAX_E * MOE_MAX_T <= 64,
              "a wave holds one (task, expert) entry per lane");

struct TaskMasks {
  unsigned m[MOE_MAX_T];  // bit e of m[t]: task t mixes expert e
};

// Store one wave's 16 x 64 tile of bf16 values (D layout: v[t][i] is column
// n0 + 16 t + lane%16, row m0 + 4*(lane/16) + i) into C[M, N]. A full tile
// goes through the wave's LDS stage and leaves as 128-B row bursts, as in
// k_linear_fwd_t; a ragged one is stored element-wise within M and N. The
// stage is the wave's own, and LDS operations of one wave execute in
// order, so it can be reused tile after tile without a barrier.
__device__ __forceinline__ void store_tile_u16(const short (&v)[4][4],
                                               int lane, int m0, int n0,
                                               int M, int N,
                                               short* __restrict__ C,
                                               short (*stage)[72]) {
  if (n0 + 64 <= N && m0 + 16 <= M && (N & 7) == 0) {  // wave-uniform
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        stage[(lane >> 4) * 4 + i][t * 16 + (lane & 15)] = v[t][i];
    __builtin_amdgcn_s_waitcnt(0);  // LDS writes visible within the wave
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int row = half * 8 + (lane >> 3);
      const int c8 = (lane & 7) * 8;
      bf16x8 vreg;
#pragma unroll
      for (int j = 0; j < 8; ++j) vreg[j] = stage[row][c8 + j];
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

// act(acc + bias) of a wave's accumulator tile, the values linear_fwd
// stores; columns past N get a zero bias and are never stored
__device__ __forceinline__ void fwd_act_tile(const f32x4 (&acc)[1][4],
                                             const float* __restrict__ bias,
                                             int lane, int n0, int N, int act,
                                             short (&v)[4][4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cn = n0 + t * 16 + (lane & 15);
    const float bv = cn < N ? bias[cn] : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[t][i] = fwd_act_u16(acc[0][t][i], bv, act);
  }
}

// ------------------------------------------------------------------
// C[e] = act(A[e] @ W[e]^T + bias[e]) for e = blockIdx.z. Block and wave
// tile of k_linear_fwd_t<1>: 4 waves stacked on M, 16 rows x 64 columns
// each. a_stride = 0 shares one A[M, K] among the experts (first layer).
// ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_expert_fwd(
    const short* __restrict__ A, int64_t a_stride,
    const short* __restrict__ W, const float* __restrict__ bias, int M, int N,
    int K, int act, short* __restrict__ C) {
  __shared__ short cstage[4][16][72];  // 72 = 64 + 8 (bank de-phase)
  const int e = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ntiles64 = (N + 63) / 64;
  const int m0 = (blockIdx.x / ntiles64) * 64 + wave * 16;
  const int n0 = (blockIdx.x % ntiles64) * 64;
  if (m0 >= M) return;
  A += e * a_stride;
  W += (int64_t)e * N * K;
  f32x4 acc[1][4] = {};
  if (m0 + 16 <= M && n0 + 64 <= N)  // wave-uniform
    fwd_accumulate<1, false>(A, W, M, N, K, m0, n0, lane, acc);
  else
    fwd_accumulate<1, true>(A, W, M, N, K, m0, n0, lane, acc);
  short v[4][4];
  fwd_act_tile(acc, bias + (int64_t)e * N, lane, n0, N, act, v);
  store_tile_u16(v, lane, m0, n0, M, N, C + (int64_t)e * M * N,
                 cstage[wave]);
}

// ------------------------------------------------------------------
// The last expert layer and the gate mixture:
//   ex[e]  = bf(act(A[e] @ W[e]^T + bias[e]))                  [E, M, N]
//   p[b,t,.] = softmax of gate[b,t,.] over the experts of task t
//   mix[t] = bf(sum_e p[.,t,e] * ex[e]), fp32 fma in ascending e [T, M, N]
// A wave owns 16 rows x 64 columns and loops over the experts: per expert
// one zeroed accumulator and the forward K loop, then v = ex's value in
// registers, then one fma per task that mixes the expert. Before the loop
// the wave computes p for its 16 rows (lane -> row lane%16, task lane/16;
// max-subtracted, fp32, masked entries exactly 0) into its own LDS tile;
// the waves of column block 0 also store it. ex and p are written only
// when their pointers are set (training).
// ------------------------------------------------------------------
template <int T>
__global__ void __launch_bounds__(256) k_expert_mix_fwd(
    const short* __restrict__ A, int64_t a_stride,
    const short* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ gate, TaskMasks tm, int E, int M, int N, int K,
    int act, short* __restrict__ mix, short* __restrict__ ex,
    float* __restrict__ p_out) {
  __shared__ short cstage[4][16][72];
  __shared__ float pl[4][16 * T * MOE_MAX_E];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ntiles64 = (N + 63) / 64;
  const int m0 = (blockIdx.x / ntiles64) * 64 + wave * 16;
  const int n0 = (blockIdx.x % ntiles64) * 64;
  if (m0 >= M) return;
  float* pw = pl[wave];  // [16][T][E]
  {
    const int r = lane & 15, t = lane >> 4, row = m0 + r;
    if (t < T) {
      const unsigned mk = tm.m[t];
      float* dst = pw + (r * T + t) * E;
      if (row < M) {
        const float* src = gate + ((int64_t)row * T + t) * E;
        float mx = -3.4e38f;
        for (int e = 0; e < E; ++e)
          if ((mk >> e) & 1) mx = fmaxf(mx, src[e]);
        float sum = 0.0f;
        for (int e = 0; e < E; ++e) {
          const float ev = ((mk >> e) & 1) ? __expf(src[e] - mx) : 0.0f;
          dst[e] = ev;
          sum += ev;
        }
        const float inv = 1.0f / sum;
        for (int e = 0; e < E; ++e) {
          const float pv = dst[e] * inv;
          dst[e] = pv;
          if (p_out && n0 == 0) p_out[((int64_t)row * T + t) * E + e] = pv;
        }
      } else {
        for (int e = 0; e < E; ++e) dst[e] = 0.0f;
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(0);  // LDS writes visible within the wave
  const bool interior = m0 + 16 <= M && n0 + 64 <= N;  // wave-uniform
  const int prow = (lane >> 4) * 4;  // first of this lane's 4 tile rows
  float mixacc[T][4][4] = {};
  for (int e = 0; e < E; ++e) {
    const short* Ae = A + e * a_stride;
    const short* We = W + (int64_t)e * N * K;
    f32x4 acc[1][4] = {};
    if (interior)
      fwd_accumulate<1, false>(Ae, We, M, N, K, m0, n0, lane, acc);
    else
      fwd_accumulate<1, true>(Ae, We, M, N, K, m0, n0, lane, acc);
    short v[4][4];
    fwd_act_tile(acc, bias + (int64_t)e * N, lane, n0, N, act, v);
    if (ex)
      store_tile_u16(v, lane, m0, n0, M, N, ex + (int64_t)e * M * N,
                     cstage[wave]);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (!((tm.m[t] >> e) & 1)) continue;  // scalar: skipped, not zeroed
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = pw[((prow + i) * T + t) * E + e];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          mixacc[t][c][i] = fmaf(pv, bf2f_u16(v[c][i]), mixacc[t][c][i]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    short o[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[c][i] = f2bf_u16(mixacc[t][c][i]);
    store_tile_u16(o, lane, m0, n0, M, N, mix + (int64_t)t * M * N,
                   cstage[wave]);
  }
}

// fixed-order butterfly: every lane ends with the same sum, the same bits
// on every run
__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------
// Backward of the mixture, one wave per sample row b (4 rows per block):
//   dpre[e,h] = bf(sum_t p[b,t,e] dmix[t,b,h])   tasks that mix e, asc. t
//   dex[e,b,h] = act_grad(dpre, ex[e,b,h])       the rule of act_grad_u16
//   dp[t,e]   = sum_h dmix[t,b,h] ex[e,b,h]
//   dgate[b,t,e] = p (dp - sum_e' p dp)          masked entries exactly 0
// Lane l < T*E owns entry (t, e) = (l / E, l % E) of p, dp and dgate; p is
// broadcast from there with wave shuffles. A lane sums its columns
// h = lane, lane + 64, ... in ascending order, then the butterfly.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_expert_mix_bwd(
    const short* __restrict__ dmix, const float* __restrict__ p,
    const short* __restrict__ ex, TaskMasks tm, int E, int T, int B, int H,
    int act, short* __restrict__ dex, float* __restrict__ dgate) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform: the shuffles below see a full wave
  const int te = T * E;
  const float pv = lane < te ? p[(int64_t)b * te + lane] : 0.0f;
  float mydp = 0.0f;
  for (int e = 0; e < E; ++e) {
    float pe[MOE_MAX_T], dpa[MOE_MAX_T];
    bool on[MOE_MAX_T];
#pragma unroll
    for (int t = 0; t < MOE_MAX_T; ++t) {
      on[t] = t < T && ((tm.m[t] >> e) & 1);
      pe[t] = __shfl(pv, on[t] ? t * E + e : 0);
      dpa[t] = 0.0f;
    }
    const int64_t erow = ((int64_t)e * B + b) * H;
    for (int hc = 0; hc < H; hc += 64) {
      const int h = hc + lane;
      const bool ok = h < H;
      const short exs = ok ? ex[erow + h] : (short)0;
      const float exv = bf2f_u16(exs);
      float dpre = 0.0f;
#pragma unroll
      for (int t = 0; t < MOE_MAX_T; ++t) {
        if (!on[t]) continue;
        const float dm =
            ok ? bf2f_u16(dmix[((int64_t)t * B + b) * H + h]) : 0.0f;
        dpre = fmaf(pe[t], dm, dpre);
        dpa[t] = fmaf(dm, exv, dpa[t]);
      }
      if (ok) {
        short g = f2bf_u16(dpre);
        if (act != 0) g = act_grad_u16(g, exs, act);
        dex[erow + h] = g;
      }
    }
#pragma unroll
    for (int t = 0; t < MOE_MAX_T; ++t) {
      if (!on[t]) continue;  // wave-uniform
      const float s = wave_sum_xor(dpa[t]);
      if (lane == t * E + e) mydp = s;
    }
  }
  const int base = lane < te ? (lane / E) * E : 0;
  const float prod = pv * mydp;  // 0 on masked entries and idle lanes
  float s = 0.0f;
  for (int e = 0; e < E; ++e) s += __shfl(prod, base + e);
  if (lane < te) {
    const bool live = (tm.m[lane / E] >> (lane % E)) & 1;
    dgate[(int64_t)b * te + lane] = live ? pv * (mydp - s) : 0.0f;
  }
}

// ------------------------------------------------------------------
// dX[e] = G[e] @ W[e] with the mapping of k_linear_dx (direct fragments, a
// 16 x 64 tile per wave). reduce = 0: the expert is grid z, dX is
// [E, M, K] and prev_out [E, M, K], when set, is applied as dx_store_tile
// applies it. reduce = 1: one accumulator runs over all experts and the
// tile is rounded once, dX[M, K] = bf(sum_e G[e] @ W[e]) — the gradient
// of an input the experts share.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_expert_dx(
    const short* __restrict__ G, const short* __restrict__ W, int E, int M,
    int N, int K, int reduce, short* __restrict__ dX,
    const short* __restrict__ prev_out, int prev_act) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ktiles64 = (K + 63) / 64;
  const int m0 = (blockIdx.x / ktiles64) * 64 + wave * 16;
  const int c0 = (blockIdx.x % ktiles64) * 64;
  if (m0 >= M) return;
  const int e0 = reduce ? 0 : blockIdx.z;
  const int e1 = reduce ? E : e0 + 1;
  const int row_g = m0 + (lane & 15);
  const int col_w = c0 + (lane & 15);
  const int kgrp = (lane >> 4) * 8;
  f32x4 acc[4] = {};
  const int kt = min(4, (K - c0 + 15) / 16);
  for (int e = e0; e < e1; ++e) {
    const short* Ge = G + (int64_t)e * M * N;
    const short* We = W + (int64_t)e * N * K;
    for (int n0 = 0; n0 < N; n0 += 32) {
      bf16x8 a = load_frag_row(Ge, row_g, n0 + kgrp, M, N);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t >= kt) break;
        bf16x8 bfrag = load_frag_col(We, col_w + t * 16, n0 + kgrp, N, K);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, acc[t], 0,
                                                         0, 0);
      }
    }
  }
  if (!reduce) {
    dX += (int64_t)e0 * M * K;
    if (prev_out) prev_out += (int64_t)e0 * M * K;
  }
  dx_store_tile(acc, lane, m0, c0, kt, M, K, dX, prev_out, prev_act);
}

}  // namespace

// ---------------------- host wrappers ----------------------

static const short* bf_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr<at::BFloat16>());
}
static short* bf_ptr_mut(torch::Tensor& t) {
  return reinterpret_cast<short*>(t.data_ptr<at::BFloat16>());
}

// The kernels index their operands as dense row-major stacks of one dtype
// on one device; anything else is rejected before a launch.
static void check_stack(const torch::Tensor& t, c10::ScalarType dtype,
                        std::initializer_list<int64_t> shape,
                        const torch::Device& dev, const char* op,
                        const char* name) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.device() == dev, op, ": ", name, " is on ", t.device(),
              ", expected ", dev);
  TORCH_CHECK(t.scalar_type() == dtype, op, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(t.sizes() == c10::IntArrayRef(shape.begin(), shape.size()), op,
              ": ", name, " is ", t.sizes(), ", expected ",
              c10::IntArrayRef(shape.begin(), shape.size()));
}

static void check_act(int64_t act, const char* op) {
  TORCH_CHECK(act >= 0 && act <= 2, op,
              ": act must be 0 (none), 1 (relu) or 2 (sigmoid), got ", act);
}

// The kernels count rows, columns and elements of one slab in int.
static void check_extent(int64_t rows, int64_t a, int64_t b, const char* op) {
  TORCH_CHECK(rows < (1 << 30) && rows * a < (1LL << 31) &&
                  rows * b < (1LL << 31) && a * b < (1LL << 31),
              op, ": a slab must stay below 2^31 elements");
}

// weights [E, N, K] bf16 and the activation operand, [B, K] shared by all
// experts or [E, B, K]; returns the operand's expert stride in elements
static int64_t check_expert_operands(const char* op, const torch::Tensor& a,
                                     const torch::Tensor& w,
                                     const torch::Tensor& bias) {
  TORCH_CHECK(w.dim() == 3, op, ": w must be [E,N,K], got ", w.dim(), "-D");
  const int64_t E = w.size(0), N = w.size(1), K = w.size(2);
  TORCH_CHECK(E >= 1 && E <= MOE_MAX_E, op, ": E must be in [1, ", MOE_MAX_E,
              "], got ", E);
  TORCH_CHECK(N >= 1 && K >= 1, op, ": empty weight");
  TORCH_CHECK(a.dim() == 2 || a.dim() == 3, op,
              ": a must be [B,K] or [E,B,K], got ", a.dim(), "-D");
  const int64_t B = a.size(a.dim() - 2);
  const torch::Device dev = a.device();
  if (a.dim() == 2)
    check_stack(a, torch::kBFloat16, {B, K}, dev, op, "a");
  else
    check_stack(a, torch::kBFloat16, {E, B, K}, dev, op, "a");
  check_stack(w, torch::kBFloat16, {E, N, K}, dev, op, "w");
  check_stack(bias, torch::kFloat32, {E, N}, dev, op, "bias");
  check_extent(B, N, K, op);
  return a.dim() == 2 ? 0 : B * K;
}

// mask [T, E] uint8 on the host -> one bit set per task
static TaskMasks pack_masks(const torch::Tensor& mask, int64_t E,
                            const char* op) {
  TORCH_CHECK(!mask.is_cuda() && mask.scalar_type() == torch::kUInt8 &&
                  mask.dim() == 2 && mask.is_contiguous(),
              op, ": mask must be a contiguous [T,E] uint8 host tensor");
  const int64_t T = mask.size(0);
  TORCH_CHECK(T >= 1 && T <= MOE_MAX_T, op, ": T must be in [1, ", MOE_MAX_T,
              "], got ", T);
  TORCH_CHECK(mask.size(1) == E, op, ": mask is [T,", mask.size(1),
              "] but there are ", E, " experts");
  TaskMasks tm = {};
  const uint8_t* mp = mask.data_ptr<uint8_t>();
  for (int64_t t = 0; t < T; ++t) {
    for (int64_t e = 0; e < E; ++e)
      if (mp[t * E + e]) tm.m[t] |= 1u << e;
    TORCH_CHECK(tm.m[t] != 0, op, ": task ", t, " mixes no expert");
  }
  return tm;
}

torch::Tensor expert_fwd(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                         int64_t act) {
  const char* op = "expert_fwd";
  check_act(act, op);
  const int64_t a_stride = check_expert_operands(op, a, w, bias);
  const int64_t E = w.size(0), N = w.size(1), K = w.size(2);
  const int64_t B = a.size(a.dim() - 2);
  auto out = torch::empty({E, B, N}, a.options());
  if (B == 0) return out;
  const dim3 grid((unsigned)(((B + 63) / 64) * ((N + 63) / 64)), 1,
                  (unsigned)E);
  k_expert_fwd<<<grid, 256, 0, current_hip_stream()>>>(
      bf_ptr(a), a_stride, bf_ptr(w), bias.data_ptr<float>(), (int)B, (int)N,
      (int)K, (int)act, bf_ptr_mut(out));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// -> (mix [T,B,H] bf16, ex [E,B,H] bf16, p [B,T,E] fp32); ex and p are
// empty without save
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> expert_mix_fwd(
    torch::Tensor a, torch::Tensor w, torch::Tensor bias, int64_t act,
    torch::Tensor gate_logits, torch::Tensor mask, bool save) {
  const char* op = "expert_mix_fwd";
  check_act(act, op);
  const int64_t a_stride = check_expert_operands(op, a, w, bias);
  const int64_t E = w.size(0), H = w.size(1), K = w.size(2);
  const int64_t B = a.size(a.dim() - 2);
  const TaskMasks tm = pack_masks(mask, E, op);
  const int64_t T = mask.size(0);
  check_stack(gate_logits, torch::kFloat32, {B, T, E}, a.device(), op,
              "gate_logits");
  auto mix = torch::empty({T, B, H}, a.options());
  auto ex = torch::empty({save ? E : 0, B, H}, a.options());
  auto p = torch::empty({save ? B : 0, T, E}, gate_logits.options());
  if (B == 0) return {mix, ex, p};
  const int blocks = (int)(((B + 63) / 64) * ((H + 63) / 64));
#define MOE_MIX_FWD(TV)                                                     \
  k_expert_mix_fwd<TV><<<blocks, 256, 0, current_hip_stream()>>>(           \
      bf_ptr(a), a_stride, bf_ptr(w), bias.data_ptr<float>(),               \
      gate_logits.data_ptr<float>(), tm, (int)E, (int)B, (int)H, (int)K,    \
      (int)act, bf_ptr_mut(mix), save ? bf_ptr_mut(ex) : nullptr,           \
      save ? p.data_ptr<float>() : nullptr)
  if (T == 1) MOE_MIX_FWD(1);
  else if (T == 2) MOE_MIX_FWD(2);
  else if (T == 3) MOE_MIX_FWD(3);
  else MOE_MIX_FWD(4);
#undef MOE_MIX_FWD
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {mix, ex, p};
}

// -> (dex [E,B,H] bf16, dgate [B,T,E] fp32)
std::tuple<torch::Tensor, torch::Tensor> expert_mix_bwd(
    torch::Tensor dmix, torch::Tensor p, torch::Tensor ex, torch::Tensor mask,
    int64_t act) {
  const char* op = "expert_mix_bwd";
  check_act(act, op);
  TORCH_CHECK(ex.dim() == 3, op, ": ex must be [E,B,H], got ", ex.dim(),
              "-D");
  const int64_t E = ex.size(0), B = ex.size(1), H = ex.size(2);
  TORCH_CHECK(E >= 1 && E <= MOE_MAX_E, op, ": E must be in [1, ", MOE_MAX_E,
              "], got ", E);
  const TaskMasks tm = pack_masks(mask, E, op);
  const int64_t T = mask.size(0);
  const torch::Device dev = ex.device();
  check_stack(ex, torch::kBFloat16, {E, B, H}, dev, op, "ex");
  check_stack(dmix, torch::kBFloat16, {T, B, H}, dev, op, "dmix");
  check_stack(p, torch::kFloat32, {B, T, E}, dev, op, "p");
  check_extent(B, H, 1, op);
  auto dex = torch::empty_like(ex);
  auto dgate = torch::empty_like(p);
  if (B == 0) return {dex, dgate};
  k_expert_mix_bwd<<<(int)((B + 3) / 4), 256, 0, current_hip_stream()>>>(
      bf_ptr(dmix), p.data_ptr<float>(), bf_ptr(ex), tm, (int)E, (int)T,
      (int)B, (int)H, (int)act, bf_ptr_mut(dex), dgate.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dex, dgate};
}

// reduce = false -> [E,B,K], with prev_out [E,B,K] / prev_act applied as in
// linear_dx; reduce = true -> [B,K], the sum over the experts rounded once
torch::Tensor expert_dx(torch::Tensor g, torch::Tensor w,
                        c10::optional<torch::Tensor> prev_out,
                        int64_t prev_act, bool reduce) {
  const char* op = "expert_dx";
  check_act(prev_act, op);
  TORCH_CHECK(g.dim() == 3 && w.dim() == 3, op,
              ": g must be [E,B,N] and w [E,N,K]");
  const int64_t E = w.size(0), N = w.size(1), K = w.size(2);
  const int64_t B = g.size(1);
  TORCH_CHECK(E >= 1 && E <= MOE_MAX_E, op, ": E must be in [1, ", MOE_MAX_E,
              "], got ", E);
  TORCH_CHECK(N >= 1 && K >= 1, op, ": empty weight");
  const torch::Device dev = g.device();
  check_stack(g, torch::kBFloat16, {E, B, N}, dev, op, "g");
  check_stack(w, torch::kBFloat16, {E, N, K}, dev, op, "w");
  check_extent(B, N, K, op);
  const short* pp = nullptr;
  if (prev_out.has_value()) {
    TORCH_CHECK(!reduce, op, ": prev_out does not apply to reduce");
    check_stack(*prev_out, torch::kBFloat16, {E, B, K}, dev, op, "prev_out");
    if (prev_act != 0) pp = bf_ptr(*prev_out);
  } else {
    TORCH_CHECK(prev_act == 0, op, ": prev_act without prev_out");
  }
  auto dx = reduce ? torch::empty({B, K}, g.options())
                   : torch::empty({E, B, K}, g.options());
  if (B == 0) return dx;
  const dim3 grid((unsigned)(((B + 63) / 64) * ((K + 63) / 64)), 1,
                  (unsigned)(reduce ? 1 : E));
  k_expert_dx<<<grid, 256, 0, current_hip_stream()>>>(
      bf_ptr(g), bf_ptr(w), (int)E, (int)B, (int)N, (int)K, reduce ? 1 : 0,
      bf_ptr_mut(dx), pp, (int)prev_act);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dx;
}

void register_moe(py::module_& mod) {
  mod.def("expert_fwd", &expert_fwd, py::arg("a"), py::arg("w"),
          py::arg("bias"), py::arg("act"));
  mod.def("expert_mix_fwd", &expert_mix_fwd, py::arg("a"), py::arg("w"),
          py::arg("bias"), py::arg("act"), py::arg("gate_logits"),
          py::arg("mask"), py::arg("save"));
  mod.def("expert_mix_bwd", &expert_mix_bwd, py::arg("dmix"), py::arg("p"),
          py::arg("ex"), py::arg("mask"), py::arg("act"));
  mod.def("expert_dx", &expert_dx, py::arg("g"), py::arg("w"),
          py::arg("prev_out") = py::none(), py::arg("prev_act") = 0,
          py::arg("reduce") = false);
}
