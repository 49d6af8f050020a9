// attention_kernels.hip — fused multi-head attention for short behavior
// sequences (MI355X / gfx950).
//
// The sequence models (DIN/BST, reference modelzoo/bst + din attention
// blocks) attend over T ≈ 50-100 items at d_model ≈ 32-64 — shapes where
// library attention (batched GEMMs + separate softmax/mask kernels) is
// pure launch overhead. CDNA4-first design instead: ONE workgroup per
// sample holds the whole sequence in LDS (K/V ≈ a few KB at these
// shapes), each thread owns one (query row, head) pair and produces its
// output row without any inter-thread communication, and the backward
// recomputes softmax from saved per-row (max, sum) stats instead of
// materializing [B, h, T, T] probabilities (170 MB at batch 8192).
//
// Capability ≙ the reference's transformer/attention blocks
// (modelzoo/bst/train.py, modelzoo/din/train.py:207-253 attention); the
// kernel design is new for this engine.

#include "hip_common.h"

#include <c10/hip/HIPException.h>

namespace {

constexpr int kMaxDh = 32;  // head dim cap (template dispatch below)

// Forward: one workgroup per sample. Threads cover (q_row, head) pairs.
// q/k/v: [B, T, D] bf16; key_pad: [B, T] uint8 (1 = masked key);
// out: [B, T, D] bf16; stats: [B, h, T, 2] fp32 (row max, row exp-sum).
// DH is a compile-time head dim so the per-thread accumulators are
// exact-size register arrays with fully unrolled loops (a kMaxDh-sized
// runtime-bounded array cost ~200 VGPRs and 4x the runtime).
template <int DH>
__global__ void k_mha_fwd(const short* __restrict__ q,
                          const short* __restrict__ k,
                          const short* __restrict__ v,
                          const uint8_t* __restrict__ key_pad, int B, int T,
                          int D, int H, float scale,
                          short* __restrict__ out,
                          float* __restrict__ stats) {
  extern __shared__ short lds[];
  short* K = lds;            // [T, D]
  short* V = lds + T * D;    // [T, D]
  const int b = blockIdx.x;
  constexpr int dh = DH;
  const int64_t base = (int64_t)b * T * D;
  for (int i = threadIdx.x; i < T * D; i += blockDim.x) {
    K[i] = k[base + i];
    V[i] = v[base + i];
  }
  __syncthreads();
  const uint8_t* pad = key_pad + (int64_t)b * T;
  for (int pair = threadIdx.x; pair < T * H; pair += blockDim.x) {
    const int qr = pair / H;
    const int h = pair % H;
    float qv[DH];
    const short* qp = q + base + (int64_t)qr * D + h * dh;
#pragma unroll
    for (int d = 0; d < dh; ++d) qv[d] = bf2f_u16(qp[d]);
    // pass 1: row max
    float mx = -1e30f;
    for (int t = 0; t < T; ++t) {
      if (pad[t]) continue;
      const short* kp = K + t * D + h * dh;
      float s = 0.0f;
      for (int d = 0; d < dh; ++d) s += qv[d] * bf2f_u16(kp[d]);
      s *= scale;
      mx = fmaxf(mx, s);
    }
    // pass 2: exp-sum + weighted V accumulation
    float acc[DH];
#pragma unroll
    for (int d = 0; d < dh; ++d) acc[d] = 0.0f;
    float sum = 0.0f;
    for (int t = 0; t < T; ++t) {
      if (pad[t]) continue;
      const short* kp = K + t * D + h * dh;
      float s = 0.0f;
      for (int d = 0; d < dh; ++d) s += qv[d] * bf2f_u16(kp[d]);
      float p = __expf(s * scale - mx);
      sum += p;
      const short* vp = V + t * D + h * dh;
      for (int d = 0; d < dh; ++d) acc[d] += p * bf2f_u16(vp[d]);
    }
    const float inv = 1.0f / fmaxf(sum, 1e-20f);
    short* op = out + base + (int64_t)qr * D + h * dh;
    for (int d = 0; d < dh; ++d) op[d] = f2bf_u16(acc[d] * inv);
    float* st = stats + (((int64_t)b * H + h) * T + qr) * 2;
    st[0] = mx;
    st[1] = sum;
  }
}

// Backward: recompute probabilities from stats; two phases per block.
// Phase A (q rows): dQ + per-row dot sum_t p*dP. Phase B (k rows):
// dK, dV. Each thread owns one output row — no atomics anywhere.
template <int DH>
__global__ void k_mha_bwd(const short* __restrict__ dout,
                          const short* __restrict__ q,
                          const short* __restrict__ k,
                          const short* __restrict__ v,
                          const uint8_t* __restrict__ key_pad,
                          const float* __restrict__ stats, int B, int T,
                          int D, int H, float scale,
                          short* __restrict__ dq, short* __restrict__ dk,
                          short* __restrict__ dv) {
  extern __shared__ short lds[];
  short* Q = lds;                       // [T, D]
  short* K = lds + T * D;               // [T, D]
  short* V = lds + 2 * T * D;           // [T, D]
  short* dO = lds + 3 * T * D;          // [T, D]
  float* row_dot = reinterpret_cast<float*>(lds + 4 * T * D);  // [T*H]
  const int b = blockIdx.x;
  constexpr int dh = DH;
  const int64_t base = (int64_t)b * T * D;
  for (int i = threadIdx.x; i < T * D; i += blockDim.x) {
    Q[i] = q[base + i];
    K[i] = k[base + i];
    V[i] = v[base + i];
    dO[i] = dout[base + i];
  }
  __syncthreads();
  const uint8_t* pad = key_pad + (int64_t)b * T;
  const float* st_b = stats + (int64_t)b * H * T * 2;
  // phase A: per (q, head): row_dot and dQ
  for (int pair = threadIdx.x; pair < T * H; pair += blockDim.x) {
    const int qr = pair / H;
    const int h = pair % H;
    const float* st = st_b + ((int64_t)h * T + qr) * 2;
    const float mx = st[0];
    const float inv = 1.0f / fmaxf(st[1], 1e-20f);
    float qv[DH], go[DH];
#pragma unroll
    for (int d = 0; d < dh; ++d) {
      qv[d] = bf2f_u16(Q[qr * D + h * dh + d]);
      go[d] = bf2f_u16(dO[qr * D + h * dh + d]);
    }
    float rd = 0.0f;
    for (int t = 0; t < T; ++t) {
      if (pad[t]) continue;
      float s = 0.0f, dp = 0.0f;
      const short* kp = K + t * D + h * dh;
      const short* vp = V + t * D + h * dh;
      for (int d = 0; d < dh; ++d) {
        s += qv[d] * bf2f_u16(kp[d]);
        dp += go[d] * bf2f_u16(vp[d]);
      }
      rd += __expf(s * scale - mx) * inv * dp;
    }
    row_dot[qr * H + h] = rd;
    float dqv[DH];
#pragma unroll
    for (int d = 0; d < dh; ++d) dqv[d] = 0.0f;
    for (int t = 0; t < T; ++t) {
      if (pad[t]) continue;
      float s = 0.0f, dp = 0.0f;
      const short* kp = K + t * D + h * dh;
      const short* vp = V + t * D + h * dh;
      for (int d = 0; d < dh; ++d) {
        s += qv[d] * bf2f_u16(kp[d]);
        dp += go[d] * bf2f_u16(vp[d]);
      }
      float p = __expf(s * scale - mx) * inv;
      float ds = p * (dp - rd) * scale;
      for (int d = 0; d < dh; ++d) dqv[d] += ds * bf2f_u16(kp[d]);
    }
    short* dqp = dq + base + (int64_t)qr * D + h * dh;
    for (int d = 0; d < dh; ++d) dqp[d] = f2bf_u16(dqv[d]);
  }
  __syncthreads();
  // phase B: per (key row, head): dK, dV
  for (int pair = threadIdx.x; pair < T * H; pair += blockDim.x) {
    const int t = pair / H;
    const int h = pair % H;
    short* dkp = dk + base + (int64_t)t * D + h * dh;
    short* dvp = dv + base + (int64_t)t * D + h * dh;
    if (pad[t]) {
      for (int d = 0; d < dh; ++d) {
        dkp[d] = 0;
        dvp[d] = 0;
      }
      continue;
    }
    float kv[DH], vv[DH], dkv[DH], dvv[DH];
#pragma unroll
    for (int d = 0; d < dh; ++d) {
      kv[d] = bf2f_u16(K[t * D + h * dh + d]);
      vv[d] = bf2f_u16(V[t * D + h * dh + d]);
      dkv[d] = 0.0f;
      dvv[d] = 0.0f;
    }
    for (int qr = 0; qr < T; ++qr) {
      const float* st = st_b + ((int64_t)h * T + qr) * 2;
      const float mx = st[0];
      const float inv = 1.0f / fmaxf(st[1], 1e-20f);
      float s = 0.0f, dp = 0.0f;
      const short* qp = Q + qr * D + h * dh;
      const short* gp = dO + qr * D + h * dh;
      for (int d = 0; d < dh; ++d) {
        s += bf2f_u16(qp[d]) * kv[d];
        dp += bf2f_u16(gp[d]) * vv[d];
      }
      float p = __expf(s * scale - mx) * inv;
      float ds = p * (dp - row_dot[qr * H + h]) * scale;
      for (int d = 0; d < dh; ++d) {
        dkv[d] += ds * bf2f_u16(qp[d]);
        dvv[d] += p * bf2f_u16(gp[d]);
      }
    }
    for (int d = 0; d < dh; ++d) {
      dkp[d] = f2bf_u16(dkv[d]);
      dvp[d] = f2bf_u16(dvv[d]);
    }
  }
}

// ---------------------------------------------------------------------
// DIN attention features: att_in[b,t] = [s, tgt, s - tgt, s * tgt]
// built in ONE pass (the torch path materializes the expand, two
// elementwise intermediates and a 4-way cat — 5 kernels and ~2x the
// HBM traffic at [B, T, 4D]). ≙ modelzoo/din/train.py attention input.
__global__ void k_din_feat_fwd(const float* __restrict__ seq,
                               const float* __restrict__ tgt, int B, int T,
                               int D, short* __restrict__ out) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = (int64_t)B * T * D;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < total; i += stride) {
    int d = (int)(i % D);
    int64_t bt = i / D;
    int b = (int)(bt / T);
    float s = seq[i];
    float t = tgt[(int64_t)b * D + d];
    short* o = out + bt * 4 * D + d;
    o[0] = f2bf_u16(s);
    o[D] = f2bf_u16(t);
    o[2 * D] = f2bf_u16(s - t);
    o[3 * D] = f2bf_u16(s * t);
  }
}

// backward: ds = g0 + g2 + g3*t (elementwise); dt[b] = sum_t
// (g1 - g2 + g3*s) via one thread per (b, d) looping T — NO atomics
// (the per-element atomicAdd variant measured 132 us/step at B*T*D
// 13M atomics).
__global__ void k_din_feat_bwd_ds(const short* __restrict__ g,
                                  const float* __restrict__ tgt, int B,
                                  int T, int D,
                                  float* __restrict__ dseq) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = (int64_t)B * T * D;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < total; i += stride) {
    int d = (int)(i % D);
    int64_t bt = i / D;
    int b = (int)(bt / T);
    const short* gp = g + bt * 4 * D + d;
    dseq[i] = bf2f_u16(gp[0]) + bf2f_u16(gp[2 * D])
              + bf2f_u16(gp[3 * D]) * tgt[(int64_t)b * D + d];
  }
}

__global__ void k_din_feat_bwd_dt(const short* __restrict__ g,
                                  const float* __restrict__ seq, int B,
                                  int T, int D,
                                  float* __restrict__ dtgt) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = (int64_t)B * D;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < total; i += stride) {
    int d = (int)(i % D);
    int b = (int)(i / D);
    float acc = 0.0f;
    for (int t = 0; t < T; ++t) {
      int64_t bt = (int64_t)b * T + t;
      const short* gp = g + bt * 4 * D + d;
      acc += bf2f_u16(gp[D]) - bf2f_u16(gp[2 * D])
             + bf2f_u16(gp[3 * D]) * seq[bt * D + d];
    }
    dtgt[i] = acc;
  }
}

// ------------------------------------------------------------------
// DIN attention tail: masked softmax over scores [B, T] + weighted
// pooling of seq [B, T, D] fused into ONE kernel per direction. The
// torch chain (masked_fill, softmax, [B,T,D] broadcast-mul
// materialization, sum, + their backwards) was ~8 launches and the
// dominant torch-glue cost of the DIN step (prof_din2.csv). A fully
// masked row pools to zeros (matches "masked positions train nothing").
// ------------------------------------------------------------------
__global__ void k_msm_pool_fwd(const float* __restrict__ scores,
                               const float* __restrict__ seq,
                               const uint8_t* __restrict__ mask,
                               int B, int T, int D,
                               float* __restrict__ w_out,
                               float* __restrict__ out) {
  extern __shared__ float smw[];  // [T]
  __shared__ float red[256];
  const int b = blockIdx.x;
  if (b >= B) return;
  float lmax = -3.4e38f;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    float s = mask[b * T + t] ? scores[b * T + t] : -3.4e38f;
    smw[t] = s;
    lmax = fmaxf(lmax, s);
  }
  red[threadIdx.x] = lmax;
  __syncthreads();
  for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const float m = red[0];
  __syncthreads();
  float lsum = 0.0f;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    float e = (smw[t] <= -3.0e38f) ? 0.0f : __expf(smw[t] - m);
    smw[t] = e;
    lsum += e;
  }
  red[threadIdx.x] = lsum;
  __syncthreads();
  for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const float inv = 1.0f / (red[0] + 1e-20f);
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    smw[t] *= inv;
    w_out[b * T + t] = smw[t];
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float acc = 0.0f;
    const float* sp = seq + (int64_t)b * T * D + d;
    for (int t = 0; t < T; ++t) acc += smw[t] * sp[(int64_t)t * D];
    out[(int64_t)b * D + d] = acc;
  }
}

// dscores[t] = mask ? w[t] * (dout.seq[t] - sum_u w[u] (dout.seq[u])) : 0
// dseq[t, d] = w[t] * dout[d]
__global__ void k_msm_pool_bwd(const float* __restrict__ dout,
                               const float* __restrict__ seq,
                               const float* __restrict__ w,
                               const uint8_t* __restrict__ mask,
                               int B, int T, int D,
                               float* __restrict__ dscores,
                               float* __restrict__ dseq) {
  extern __shared__ float sdot[];  // [T] row dots, then [D] dout row
  __shared__ float red[256];
  const int b = blockIdx.x;
  if (b >= B) return;
  float* sdo = sdot + T;
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    sdo[d] = dout[(int64_t)b * D + d];
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const float* sp = seq + ((int64_t)b * T + t) * D;
    float acc = 0.0f;
    for (int d = 0; d < D; ++d) acc += sdo[d] * sp[d];
    sdot[t] = acc;
  }
  __syncthreads();
  float lw = 0.0f;
  for (int t = threadIdx.x; t < T; t += blockDim.x)
    lw += w[b * T + t] * sdot[t];
  red[threadIdx.x] = lw;
  __syncthreads();
  for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const float wdot = red[0];
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const float wt = w[b * T + t];
    dscores[b * T + t] =
        mask[b * T + t] ? wt * (sdot[t] - wdot) : 0.0f;
  }
  for (int i = threadIdx.x; i < T * D; i += blockDim.x) {
    const int t = i / D;
    dseq[(int64_t)b * T * D + i] = w[b * T + t] * sdo[i - t * D];
  }
}

}  // namespace

static const short* att_bf_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr<at::BFloat16>());
}
static short* att_bf_ptr_mut(torch::Tensor& t) {
  return reinterpret_cast<short*>(t.data_ptr<at::BFloat16>());
}

// Host-side admission for the attention launches. Both directions keep
// the whole sample in dynamic LDS, so the request grows with T*D; it is
// checked against the device's own per-block limit (queried, not assumed)
// before anything is launched, and the launch status is checked after, so
// a refused launch raises instead of handing back uninitialised tensors.
static size_t mha_lds_request(int64_t T, int64_t D, int64_t H, bool bwd) {
  const size_t tile = (size_t)T * D * sizeof(short);  // one [T, D] operand
  return bwd ? 4 * tile + (size_t)T * H * sizeof(float) : 2 * tile;
}

static int64_t mha_lds_limit_for(int device) {
  int v = 0;
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &v, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  return v;
}

int64_t mha_lds_limit() {
  int device = 0;
  C10_HIP_CHECK(hipGetDevice(&device));
  return mha_lds_limit_for(device);
}

int64_t mha_lds_bytes(int64_t T, int64_t D, int64_t H, bool bwd) {
  return (int64_t)mha_lds_request(T, D, H, bwd);
}

static void check_mha_operand(const torch::Tensor& t, const torch::Tensor& q,
                              const char* name, bool need_contiguous) {
  TORCH_CHECK(t.is_cuda() && t.get_device() == q.get_device(), "mha: ", name,
              " must be on the device of q");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, "mha: ", name,
              " must be bf16");
  TORCH_CHECK(t.sizes() == q.sizes(), "mha: ", name, " must have q's shape");
  TORCH_CHECK(!need_contiguous || t.is_contiguous(), "mha: ", name,
              " must be contiguous");
}

// shapes, dtypes and the LDS request shared by both directions
static void check_mha(const torch::Tensor& q, const torch::Tensor& k,
                      const torch::Tensor& v, const torch::Tensor& key_pad,
                      int64_t n_heads, bool bwd) {
  TORCH_CHECK(q.dim() == 3, "mha: q must be [B, T, D]");
  check_mha_operand(q, q, "q", true);
  check_mha_operand(k, q, "k", true);
  check_mha_operand(v, q, "v", true);
  const int64_t B = q.size(0), T = q.size(1), D = q.size(2);
  TORCH_CHECK(key_pad.is_cuda() && key_pad.get_device() == q.get_device(),
              "mha: key_pad must be on the device of q");
  TORCH_CHECK(key_pad.scalar_type() == torch::kUInt8,
              "mha: key_pad must be uint8");
  TORCH_CHECK(key_pad.is_contiguous() && key_pad.dim() == 2
                  && key_pad.size(0) == B && key_pad.size(1) == T,
              "mha: key_pad must be contiguous [B, T]");
  TORCH_CHECK(n_heads >= 1 && D % n_heads == 0 && D / n_heads <= kMaxDh,
              "head dim too large");
  const int64_t dh = D / n_heads;
  TORCH_CHECK(dh == 4 || dh == 8 || dh == 16 || dh == 32,
              "head dim must be 4/8/16/32");
  TORCH_CHECK(T * n_heads <= 1024,
              "sequence too long for the per-sample block");
  const int64_t need = (int64_t)mha_lds_request(T, D, n_heads, bwd);
  const int64_t limit = mha_lds_limit_for(q.get_device());
  TORCH_CHECK(need <= limit, "mha_", bwd ? "bwd" : "fwd", ": T=", T, " D=", D,
              " H=", n_heads, " needs ", need,
              " bytes of LDS per block, the device allows ", limit);
}

// A request above the default dynamic-LDS size has to be announced for
// the kernel; below it this is skipped, so the common shapes pay nothing.
template <typename K>
static void mha_allow_lds(K kernel, size_t lds) {
  if (lds > 48 * 1024) {
    C10_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
}

std::tuple<torch::Tensor, torch::Tensor> mha_fwd(torch::Tensor q,
                                                 torch::Tensor k,
                                                 torch::Tensor v,
                                                 torch::Tensor key_pad,
                                                 int64_t n_heads,
                                                 double scale) {
  check_mha(q, k, v, key_pad, n_heads, false);
  int B = q.size(0), T = q.size(1), D = q.size(2);
  int H = (int)n_heads;
  auto out = torch::empty_like(q);
  auto stats = torch::empty({B, (int64_t)H, (int64_t)T, 2},
                            q.options().dtype(torch::kFloat32));
  if (B == 0 || T == 0) return {out, stats};
  size_t lds = mha_lds_request(T, D, H, false);
  int threads = std::min(1024, ((T * H + 63) / 64) * 64);
  const int dh = D / H;
#define MHA_FWD(DHV) \
  mha_allow_lds(k_mha_fwd<DHV>, lds); \
  k_mha_fwd<DHV><<<B, threads, lds, current_hip_stream()>>>( \
      att_bf_ptr(q), att_bf_ptr(k), att_bf_ptr(v), \
      key_pad.data_ptr<uint8_t>(), B, T, D, H, (float)scale, \
      att_bf_ptr_mut(out), stats.data_ptr<float>())
  if (dh == 4) { MHA_FWD(4); }
  else if (dh == 8) { MHA_FWD(8); }
  else if (dh == 16) { MHA_FWD(16); }
  else { MHA_FWD(32); }
#undef MHA_FWD
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {out, stats};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> mha_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor key_pad, torch::Tensor stats, int64_t n_heads,
    double scale) {
  check_mha(q, k, v, key_pad, n_heads, true);
  check_mha_operand(dout, q, "dout", false);
  int B = q.size(0), T = q.size(1), D = q.size(2);
  int H = (int)n_heads;
  TORCH_CHECK(stats.is_cuda() && stats.get_device() == q.get_device()
                  && stats.scalar_type() == torch::kFloat32
                  && stats.is_contiguous() && stats.dim() == 4
                  && stats.size(0) == B && stats.size(1) == H
                  && stats.size(2) == T && stats.size(3) == 2,
              "mha_bwd: stats must be contiguous fp32 [B, H, T, 2]");
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  if (B == 0 || T == 0) return {dq, dk, dv};
  size_t lds = mha_lds_request(T, D, H, true);
  int threads = std::min(1024, ((T * H + 63) / 64) * 64);
  const int dh = D / H;
  auto dc = dout.contiguous();
#define MHA_BWD(DHV) \
  mha_allow_lds(k_mha_bwd<DHV>, lds); \
  k_mha_bwd<DHV><<<B, threads, lds, current_hip_stream()>>>( \
      att_bf_ptr(dc), att_bf_ptr(q), att_bf_ptr(k), \
      att_bf_ptr(v), key_pad.data_ptr<uint8_t>(), stats.data_ptr<float>(), \
      B, T, D, H, (float)scale, att_bf_ptr_mut(dq), att_bf_ptr_mut(dk), \
      att_bf_ptr_mut(dv))
  if (dh == 4) { MHA_BWD(4); }
  else if (dh == 8) { MHA_BWD(8); }
  else if (dh == 16) { MHA_BWD(16); }
  else { MHA_BWD(32); }
#undef MHA_BWD
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dq, dk, dv};
}

torch::Tensor din_feat_fwd(torch::Tensor seq, torch::Tensor tgt) {
  TORCH_CHECK(seq.is_contiguous() && seq.scalar_type() == torch::kFloat32);
  int B = seq.size(0), T = seq.size(1), D = seq.size(2);
  auto out = torch::empty({(int64_t)B * T, 4 * (int64_t)D},
                          seq.options().dtype(torch::kBFloat16));
  int64_t total = (int64_t)B * T * D;
  if (total == 0) return out;  // an empty grid is a launch error
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  k_din_feat_fwd<<<blocks, 256, 0, current_hip_stream()>>>(
      seq.data_ptr<float>(), tgt.data_ptr<float>(), B, T, D,
      att_bf_ptr_mut(out));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> din_feat_bwd(torch::Tensor g,
                                                      torch::Tensor seq,
                                                      torch::Tensor tgt) {
  int B = seq.size(0), T = seq.size(1), D = seq.size(2);
  auto dseq = torch::empty_like(seq);
  auto dtgt = torch::empty_like(tgt);
  auto gc = g.contiguous();
  int64_t total = (int64_t)B * T * D;
  if ((int64_t)B * D == 0) return {dseq, dtgt};
  if (total == 0) {  // T = 0: nothing to sum, dtgt is all zero
    dtgt.zero_();
    return {dseq, dtgt};
  }
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  k_din_feat_bwd_ds<<<blocks, 256, 0, current_hip_stream()>>>(
      att_bf_ptr(gc), tgt.data_ptr<float>(), B, T, D,
      dseq.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  int blocks2 = (int)std::min<int64_t>(((int64_t)B * D + 255) / 256, 8192);
  k_din_feat_bwd_dt<<<blocks2, 256, 0, current_hip_stream()>>>(
      att_bf_ptr(gc), seq.data_ptr<float>(), B, T, D,
      dtgt.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dseq, dtgt};
}

std::tuple<torch::Tensor, torch::Tensor> msm_pool_fwd(torch::Tensor scores,
                                                      torch::Tensor seq,
                                                      torch::Tensor mask) {
  TORCH_CHECK(scores.scalar_type() == torch::kFloat32
                  && scores.is_contiguous());
  TORCH_CHECK(seq.scalar_type() == torch::kFloat32 && seq.is_contiguous());
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8 && mask.is_contiguous());
  int B = scores.size(0), T = scores.size(1), D = seq.size(2);
  TORCH_CHECK(seq.size(0) == B && seq.size(1) == T && mask.numel() == B * T);
  TORCH_CHECK(T <= 4096, "sequence too long for the per-sample block");
  auto w = torch::empty_like(scores);
  auto out = torch::empty({(int64_t)B, (int64_t)D}, seq.options());
  if (B == 0) return {out, w};
  k_msm_pool_fwd<<<B, 128, (size_t)T * sizeof(float), current_hip_stream()>>>(
      scores.data_ptr<float>(), seq.data_ptr<float>(),
      mask.data_ptr<uint8_t>(), B, T, D, w.data_ptr<float>(),
      out.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {out, w};
}

std::tuple<torch::Tensor, torch::Tensor> msm_pool_bwd(torch::Tensor dout,
                                                      torch::Tensor seq,
                                                      torch::Tensor w,
                                                      torch::Tensor mask) {
  int B = seq.size(0), T = seq.size(1), D = seq.size(2);
  auto dc = dout.contiguous();
  auto dscores = torch::empty_like(w);
  auto dseq = torch::empty_like(seq);
  if (B == 0) return {dscores, dseq};
  k_msm_pool_bwd<<<B, 128, (size_t)(T + D) * sizeof(float),
                   current_hip_stream()>>>(
      dc.data_ptr<float>(), seq.data_ptr<float>(), w.data_ptr<float>(),
      mask.data_ptr<uint8_t>(), B, T, D, dscores.data_ptr<float>(),
      dseq.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dscores, dseq};
}

void register_attention(pybind11::module_& mod) {
  mod.def("mha_fwd", &mha_fwd);
  mod.def("mha_bwd", &mha_bwd);
  mod.def("mha_lds_limit", &mha_lds_limit);
  mod.def("mha_lds_bytes", &mha_lds_bytes, pybind11::arg("T"),
          pybind11::arg("D"), pybind11::arg("H"), pybind11::arg("bwd"));
  mod.def("din_feat_fwd", &din_feat_fwd);
  mod.def("din_feat_bwd", &din_feat_bwd);
  mod.def("msm_pool_fwd", &msm_pool_fwd);
  mod.def("msm_pool_bwd", &msm_pool_bwd);
}
