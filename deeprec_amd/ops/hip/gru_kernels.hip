// gru_kernels.hip — fused GRU / AUGRU recurrence for gfx950.
//
// DIEN's interest-extractor GRU and attention-gated AUGRU (reference:
// modelzoo/dien/train.py:207-253) ran through MIOpen's RNN path +
// a per-timestep python loop: 92 ms/step at B=16384,T=50,H=32, dominated
// by a 44 ms Op2dTensorSquash and ~600 launches. This replaces the whole
// recurrence with ONE kernel per direction:
//
//  - x-side projections for ALL timesteps are a single MFMA GEMM
//    (dense_kernels' linear_fwd) producing X3 = x W_ih^T + b_ih;
//  - the recurrence kernel runs one WAVE per sample: W_hh lives in LDS
//    (shared block-wide), h in per-wave LDS, 2 barriers per timestep;
//  - backward stores per-gate pre-activation grads so ALL weight/input
//    grads reduce to three linear_dx/linear_dw GEMM calls; the reverse
//    recurrence kernel only chains dh and emits dpre tensors (+ dalpha
//    for AUGRU).
//
// torch GRU gate math and weight layout (weight_ih/hh rows = [r; z; n]):
//   r = sigmoid(x_r + h U_r + bh_r)
//   z = sigmoid(x_z + h U_z + bh_z)
//   n = tanh(x_n + r * (h U_n + bh_n))
//   h' = (1-z) n + z h
// AUGRU (attention factor a): h' = (1-a) h + a ((1-z) n + z h).
// Constraints: H <= 32, 3H <= 96 (DIEN uses H=32).
//
// k_gru_tile_* further down run the same recurrence for H <= 64 on the
// matrix cores, 16 samples per wave (gru_tile_fwd / gru_tile_bwd).

#include "hip_common.h"

namespace {

constexpr int MAXH = 32;
constexpr int MAX3H = 96;

template <bool AUGRU>
__global__ void k_gru_fwd(const short* __restrict__ X3,   // [B,T,3H] bf16
                          const short* __restrict__ U,    // [3H,H] bf16
                          const float* __restrict__ bh,   // [3H]
                          const float* __restrict__ alpha,  // [B,T] | null
                          int B, int T, int H,
                          float* __restrict__ h_out,      // [B,T,H]
                          short* __restrict__ gates) {    // [B,T,3H] bf16
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  const int H3 = 3 * H;
  __shared__ short u_l[MAX3H][MAXH + 1];
  __shared__ float h_l[4][MAXH];
  __shared__ float a_l[4][MAX3H];
  for (int t = threadIdx.x; t < H3 * H; t += blockDim.x)
    u_l[t / H][t % H] = U[t];
  if (lane < H) h_l[wave][lane] = 0.0f;
  __syncthreads();

  const bool active = b < B;
  for (int t = 0; t < T; ++t) {
    // phase 1: h-side pre-activations for all 3H gates
    if (active) {
#pragma unroll 2
      for (int rep = 0; rep < 2; ++rep) {
        int g = lane + rep * 64;
        if (g < H3) {
          float s = bh[g];
          for (int k = 0; k < H; ++k)
            s += bf2f_u16(u_l[g][k]) * h_l[wave][k];
          a_l[wave][g] = s;
        }
      }
    }
    __syncthreads();
    // phase 2: gates + state update (lanes 0..H-1)
    if (active && lane < H) {
      int64_t xbase = ((int64_t)b * T + t) * H3;
      float xr = bf2f_u16(X3[xbase + lane]);
      float xz = bf2f_u16(X3[xbase + H + lane]);
      float xn = bf2f_u16(X3[xbase + 2 * H + lane]);
      float r = 1.0f / (1.0f + __expf(-(xr + a_l[wave][lane])));
      float z = 1.0f / (1.0f + __expf(-(xz + a_l[wave][H + lane])));
      float n = tanhf(xn + r * a_l[wave][2 * H + lane]);
      float h = h_l[wave][lane];
      float h_new = (1.0f - z) * n + z * h;
      if constexpr (AUGRU) {
        float a = alpha[(int64_t)b * T + t];
        h = (1.0f - a) * h + a * h_new;
      } else {
        h = h_new;
      }
      h_l[wave][lane] = h;
      int64_t obase = ((int64_t)b * T + t) * H;
      h_out[obase + lane] = h;
      gates[xbase + lane] = f2bf_u16(r);
      gates[xbase + H + lane] = f2bf_u16(z);
      gates[xbase + 2 * H + lane] = f2bf_u16(n);
    }
    __syncthreads();
  }
}

template <bool AUGRU>
__global__ void k_gru_bwd(
    const float* __restrict__ dh_out,   // [B,T,H] incoming per-step grads
    const float* __restrict__ h_out,    // [B,T,H] saved states
    const short* __restrict__ gates,    // [B,T,3H] bf16 (r,z,n)
    const short* __restrict__ U, const float* __restrict__ bh,
    const float* __restrict__ alpha, int B, int T, int H,
    short* __restrict__ dpre_x,         // [B,T,3H] bf16
    short* __restrict__ dpre_h,         // [B,T,3H] bf16 (n-part *= r)
    float* __restrict__ dalpha) {       // [B,T] | null
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  const int H3 = 3 * H;
  __shared__ short u_l[MAX3H][MAXH + 1];
  __shared__ float h_l[4][MAXH];      // h_{t-1}
  __shared__ float pn_l[4][MAXH];     // n-gate h-side preactivation
  __shared__ float dp_l[4][MAX3H];    // dpre (h-side) for transposed matvec
  __shared__ float red_l[4][MAXH];    // dalpha reduction scratch
  for (int t = threadIdx.x; t < H3 * H; t += blockDim.x)
    u_l[t / H][t % H] = U[t];
  __syncthreads();

  const bool active = b < B;
  float dh_carry = 0.0f;  // lane < H holds dh w.r.t. h_t[lane]
  for (int t = T - 1; t >= 0; --t) {
    // s1: stage h_{t-1}
    if (active && lane < H) {
      h_l[wave][lane] =
          t > 0 ? h_out[((int64_t)b * T + t - 1) * H + lane] : 0.0f;
    }
    __syncthreads();
    // s2: recompute n-gate h-side preactivation
    if (active && lane < H) {
      int g = 2 * H + lane;
      float s = bh[g];
      for (int k = 0; k < H; ++k)
        s += bf2f_u16(u_l[g][k]) * h_l[wave][k];
      pn_l[wave][lane] = s;
    }
    __syncthreads();
    // s3: cell backward -> dpre tensors (+ dalpha partial)
    float dh_prev_direct = 0.0f;
    if (active && lane < H) {
      int64_t gbase = ((int64_t)b * T + t) * H3;
      float r = bf2f_u16(gates[gbase + lane]);
      float z = bf2f_u16(gates[gbase + H + lane]);
      float n = bf2f_u16(gates[gbase + 2 * H + lane]);
      float h_prev = h_l[wave][lane];
      float dht = dh_carry + dh_out[((int64_t)b * T + t) * H + lane];
      float eff = 1.0f, da_part = 0.0f;
      if constexpr (AUGRU) {
        float a = alpha[(int64_t)b * T + t];
        float h_cand = (1.0f - z) * n + z * h_prev;
        da_part = dht * (h_cand - h_prev);
        eff = a;
      }
      float dn = dht * eff * (1.0f - z);
      float dz = dht * eff * (h_prev - n);
      dh_prev_direct = dht * ((1.0f - eff) + eff * z);
      float dpn = dn * (1.0f - n * n);
      float dpz = dz * z * (1.0f - z);
      float dr = dpn * pn_l[wave][lane];
      float dpr = dr * r * (1.0f - r);
      dpre_x[gbase + lane] = f2bf_u16(dpr);
      dpre_x[gbase + H + lane] = f2bf_u16(dpz);
      dpre_x[gbase + 2 * H + lane] = f2bf_u16(dpn);
      float dpn_h = dpn * r;
      dpre_h[gbase + lane] = f2bf_u16(dpr);
      dpre_h[gbase + H + lane] = f2bf_u16(dpz);
      dpre_h[gbase + 2 * H + lane] = f2bf_u16(dpn_h);
      dp_l[wave][lane] = dpr;
      dp_l[wave][H + lane] = dpz;
      dp_l[wave][2 * H + lane] = dpn_h;
      if constexpr (AUGRU) red_l[wave][lane] = da_part;
    }
    __syncthreads();
    // s4: dh_{t-1} = direct + dpre_h @ U (transposed matvec)
    if (active && lane < H) {
      float s = dh_prev_direct;
      for (int g = 0; g < H3; ++g)
        s += dp_l[wave][g] * bf2f_u16(u_l[g][lane]);
      dh_carry = s;
      if constexpr (AUGRU) {
        if (lane == 0) {
          float acc = 0.0f;
          for (int k = 0; k < H; ++k) acc += red_l[wave][k];
          dalpha[(int64_t)b * T + t] = acc;
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

static void check_gru(int H) {
  TORCH_CHECK(H <= MAXH, "fused GRU supports hidden size <= 32");
}

std::tuple<torch::Tensor, torch::Tensor> gru_fwd(
    torch::Tensor x3, torch::Tensor u_bf16, torch::Tensor bias_h,
    torch::Tensor alpha, int64_t B, int64_t T, int64_t H) {
  check_gru((int)H);
  auto h_out = torch::empty({B, T, H},
                            bias_h.options().dtype(torch::kFloat32));
  auto gates = torch::empty({B, T, 3 * H},
                            x3.options().dtype(torch::kBFloat16));
  int blocks = (int)((B + 3) / 4);
  auto stream = current_hip_stream();
  const bool augru = alpha.defined() && alpha.numel() > 0;
  auto* x3p = reinterpret_cast<const short*>(x3.data_ptr<at::BFloat16>());
  auto* up = reinterpret_cast<const short*>(u_bf16.data_ptr<at::BFloat16>());
  auto* gp = reinterpret_cast<short*>(gates.data_ptr<at::BFloat16>());
  if (augru) {
    k_gru_fwd<true><<<blocks, 256, 0, stream>>>(
        x3p, up, bias_h.data_ptr<float>(), alpha.data_ptr<float>(), (int)B,
        (int)T, (int)H, h_out.data_ptr<float>(), gp);
  } else {
    k_gru_fwd<false><<<blocks, 256, 0, stream>>>(
        x3p, up, bias_h.data_ptr<float>(), nullptr, (int)B, (int)T, (int)H,
        h_out.data_ptr<float>(), gp);
  }
  return {h_out, gates};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> gru_bwd(
    torch::Tensor dh_out, torch::Tensor h_out, torch::Tensor gates,
    torch::Tensor u_bf16, torch::Tensor bias_h, torch::Tensor alpha,
    int64_t B, int64_t T, int64_t H) {
  check_gru((int)H);
  auto dpre_x = torch::empty({B, T, 3 * H},
                             gates.options().dtype(torch::kBFloat16));
  auto dpre_h = torch::empty_like(dpre_x);
  const bool augru = alpha.defined() && alpha.numel() > 0;
  auto dalpha = augru
                    ? torch::empty({B, T},
                                   h_out.options().dtype(torch::kFloat32))
                    : torch::Tensor();
  int blocks = (int)((B + 3) / 4);
  auto stream = current_hip_stream();
  auto* gp = reinterpret_cast<const short*>(gates.data_ptr<at::BFloat16>());
  auto* up = reinterpret_cast<const short*>(u_bf16.data_ptr<at::BFloat16>());
  auto* dxp = reinterpret_cast<short*>(dpre_x.data_ptr<at::BFloat16>());
  auto* dhp = reinterpret_cast<short*>(dpre_h.data_ptr<at::BFloat16>());
  if (augru) {
    k_gru_bwd<true><<<blocks, 256, 0, stream>>>(
        dh_out.contiguous().data_ptr<float>(), h_out.data_ptr<float>(), gp,
        up, bias_h.data_ptr<float>(), alpha.data_ptr<float>(), (int)B,
        (int)T, (int)H, dxp, dhp, dalpha.data_ptr<float>());
  } else {
    k_gru_bwd<false><<<blocks, 256, 0, stream>>>(
        dh_out.contiguous().data_ptr<float>(), h_out.data_ptr<float>(), gp,
        up, bias_h.data_ptr<float>(), nullptr, (int)B, (int)T, (int)H, dxp,
        dhp, nullptr);
  }
  return {dpre_x, dpre_h, dalpha};
}

// ------------------------------------------------------------------
// Tile recurrence, H <= 64: 16 samples per wave on the matrix cores.
//
// A block is 4 waves; each wave owns 16 samples for all T steps, the grid
// is ceil(B / 64). The state is the A operand (rows = samples, k = hidden
// unit), W_hh the B operand of v_mfma_f32_16x16x32_bf16, staged once per
// block in LDS, zero-padded to 64 x 64 per gate. After that staging
// nothing crosses waves, so the time loop has no block barrier: a wave
// writes its operand tile to its own LDS slice and reads it back behind a
// wave-level fence (LDS serves one wave's accesses in order).
//
// Lane maps of the 16x16x32 bf16 MFMA (lane l, c = l & 15, q = l >> 4):
//   A fragment element j = A[row c][k = 8q + j]
//   B fragment element j = B[k = 8q + j][col c]
//   C/D register i       = C[row 4q + i][col c]
// so the r, z and n pre-activations of one (sample, unit) arrive in the
// same lane and register of three accumulators and the cell math needs no
// cross-lane traffic. The state stays fp32 in that layout in registers.
//
// The fp32 operand goes into the MFMA as a sum of bf16 terms, hi = bf16(v),
// lo = bf16(v - hi), ..., each multiplied in its own MFMA into the same
// fp32 accumulator, so the product keeps the precision class of k_gru_*'s
// fp32-state x bf16-weight FMAs: two terms forward (|v - hi - lo| <=
// 2^-17 |v|), three, which is exact, backward.
//
// Padding: rows of W beyond H and columns k >= H of both operands are
// real zeros (0 x NaN is NaN); tile rows with sample >= B load nothing,
// run on zeros and store nothing; columns n >= H are never stored.
// ------------------------------------------------------------------
namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TILE_MAXH = 64;
constexpr int TILE_NT = TILE_MAXH / 16;  // N tiles of 16 units per gate
constexpr int TILE_KS = TILE_MAXH / 32;  // K steps of 32
// LDS row stride in elements: 144 B keeps every 16-B fragment aligned and
// moves consecutive rows by 4 banks
constexpr int TILE_LD = TILE_MAXH + 8;
constexpr int TILE_ROWS = 16;            // samples per wave
constexpr int TILE_BLOCK_ROWS = 4 * TILE_ROWS;

// Orders one wave's LDS writes against its own later reads (and reads
// against later writes) across lanes; no other wave touches the tile.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bf16x8 lds_frag(const short* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

constexpr int TILE_PLANE = TILE_ROWS * TILE_LD;  // one bf16 term of a tile

// One wave's operand tile, TERMS planes of [16 samples][TILE_LD]: the fp32
// operand as a sum of bf16 terms, each the rounded remainder of the ones
// before it. Two terms leave at most 2^-17 |v|; three are exact (24 bits =
// 3 x 8, every remainder exact in fp32).
template <int TERMS>
struct SplitTile {
  short* base;
  int wr;  // element offset of (row 4q, col c): the accumulator layout
  int rd;  // element offset of (row c, k 8q): the A fragment
  __device__ __forceinline__ SplitTile(short* b, int lane)
      : base(b), wr(4 * (lane >> 4) * TILE_LD + (lane & 15)),
        rd((lane & 15) * TILE_LD + 8 * (lane >> 4)) {}
  // v (accumulator layout, N tile nt) -> its terms
  __device__ __forceinline__ void put(int nt, const f32x4& v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = wr + i * TILE_LD + 16 * nt;
      float rest = v[i];
#pragma unroll
      for (int p = 0; p < TERMS; ++p) {
        const short s = f2bf_u16(rest);
        base[p * TILE_PLANE + o] = s;
        rest -= bf2f_u16(s);
      }
    }
  }
  // the A fragments of K step ks, one per term
  __device__ __forceinline__ void frags(int ks, bf16x8 (&a)[TERMS]) const {
#pragma unroll
    for (int p = 0; p < TERMS; ++p)
      a[p] = lds_frag(base + p * TILE_PLANE + rd + 32 * ks);
  }
};

// acc += (a[0] + a[1] + ...) b, the largest term first
template <int TERMS>
__device__ __forceinline__ f32x4 mfma_split(const bf16x8 (&a)[TERMS],
                                            const bf16x8& b, f32x4 acc) {
#pragma unroll
  for (int p = 0; p < TERMS; ++p)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[p], b, acc, 0, 0, 0);
  return acc;
}

// big += a[0] b, small += (a[1] + ...) b: the remainder terms, 2^-8 and
// less of the leading one, sum among themselves, so that only the leading
// term's MFMAs round at the magnitude of the result. The caller adds
// `small` to `big` once at the end.
template <int TERMS>
__device__ __forceinline__ void mfma_split_apart(const bf16x8 (&a)[TERMS],
                                                 const bf16x8& b, f32x4& big,
                                                 f32x4& small) {
  big = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b, big, 0, 0, 0);
#pragma unroll
  for (int p = 1; p < TERMS; ++p)
    small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[p], b, small, 0, 0, 0);
}

constexpr int FWD_TERMS = 2;
// The backward takes all three: dh_t = carry + dh_out cancels, and what a
// two-term operand leaves of the carry and of pn then shows as several
// bf16 ulps of dpre (the fp32 model in tests/gru_tile_reference.py).
constexpr int BWD_TERMS = 3;

template <bool AUGRU>
__global__ __launch_bounds__(256) void k_gru_tile_fwd(
    const short* __restrict__ X3,     // [B,T,3H] bf16
    const short* __restrict__ U,      // [3H,H] bf16
    const float* __restrict__ bh,     // [3H]
    const float* __restrict__ alpha,  // [B,T] | null
    int B, int T, int H,
    float* __restrict__ h_out,        // [B,T,H]
    short* __restrict__ gates) {      // [B,T,3H] bf16
  // w_l[g][n][k] = U[g*H + n][k]: lane (c, q) reads B[k = 8q..][col c] of
  // N tile nt as 16 B of row 16nt + c
  __shared__ __attribute__((aligned(16))) short
      w_l[3][TILE_MAXH][TILE_LD];
  __shared__ __attribute__((aligned(16))) short
      a_l[4][FWD_TERMS * TILE_PLANE];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int H3 = 3 * H;
  const int NT = (H + 15) >> 4;
  const int KS = (H + 31) >> 5;
  for (int i = threadIdx.x; i < 3 * TILE_MAXH * TILE_LD; i += blockDim.x) {
    const int k = i % TILE_LD;
    const int n = (i / TILE_LD) % TILE_MAXH;
    const int g = i / (TILE_LD * TILE_MAXH);
    (&w_l[0][0][0])[i] = (n < H && k < H) ? U[(g * H + n) * H + k] : (short)0;
  }
  for (int i = lane; i < FWD_TERMS * TILE_PLANE; i += 64) a_l[wave][i] = 0;
  __syncthreads();

  const int col = lane & 15;
  const int row0 = blockIdx.x * TILE_BLOCK_ROWS + wave * TILE_ROWS;
  if (row0 >= B) return;  // no barrier follows
  const int srow = row0 + 4 * (lane >> 4);  // sample of register 0
  SplitTile<FWD_TERMS> tile(a_l[wave], lane);

  float bias[3][TILE_NT];
#pragma unroll
  for (int nt = 0; nt < TILE_NT; ++nt) {
    const int c = 16 * nt + col;
#pragma unroll
    for (int g = 0; g < 3; ++g) bias[g][nt] = c < H ? bh[g * H + c] : 0.0f;
  }
  f32x4 h[TILE_NT];
#pragma unroll
  for (int nt = 0; nt < TILE_NT; ++nt) h[nt] = {0.f, 0.f, 0.f, 0.f};

  // x-side pre-activations of one step in the accumulator layout; the next
  // step's are in flight while this one computes
  float xc[3][TILE_NT][4], xn[3][TILE_NT][4];
  auto load_x = [&](int t, float (&x)[3][TILE_NT][4]) {
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt) {
      if (nt < NT) {
        const int c = 16 * nt + col;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = c < H && srow + i < B;
          const int64_t base = ((int64_t)(srow + i) * T + t) * H3 + c;
#pragma unroll
          for (int g = 0; g < 3; ++g)
            x[g][nt][i] = ok ? bf2f_u16(X3[base + g * H]) : 0.0f;
        }
      }
    }
  };
  load_x(0, xc);

  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) load_x(t + 1, xn);
    float a[4];
    if constexpr (AUGRU) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = srow + i < B ? alpha[(int64_t)(srow + i) * T + t] : 0.0f;
    }
    // h_{t-1} -> A operand
    wave_lds_fence();
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt)
      if (nt < NT) tile.put(nt, h[nt]);
    wave_lds_fence();
    bf16x8 af[TILE_KS][FWD_TERMS];
#pragma unroll
    for (int ks = 0; ks < TILE_KS; ++ks)
      if (ks < KS) tile.frags(ks, af[ks]);
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt) {
      if (nt < NT) {
        f32x4 acc[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const float b0 = bias[g][nt];
          acc[g] = {b0, b0, b0, b0};
#pragma unroll
          for (int ks = 0; ks < TILE_KS; ++ks) {
            if (ks < KS) {
              const bf16x8 w =
                  lds_frag(&w_l[g][16 * nt + col][32 * ks + 8 * (lane >> 4)]);
              acc[g] = mfma_split(af[ks], w, acc[g]);
            }
          }
        }
        const int c = 16 * nt + col;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = c < H && srow + i < B;
          const float r = 1.0f / (1.0f + __expf(-(xc[0][nt][i] + acc[0][i])));
          const float z = 1.0f / (1.0f + __expf(-(xc[1][nt][i] + acc[1][i])));
          // the fused multiply-adds are spelled out so that the GRU and
          // the AUGRU instantiation round alike: alpha = 1 is the GRU and
          // alpha = 0 keeps the state, bit for bit
          const float n = tanhf(__fmaf_rn(r, acc[2][i], xc[2][nt][i]));
          float hv = h[nt][i];
          const float h_new = __fmaf_rn(z, hv, __fmul_rn(1.0f - z, n));
          if constexpr (AUGRU) {
            hv = __fmaf_rn(a[i], h_new, __fmul_rn(1.0f - a[i], hv));
          } else {
            hv = h_new;
          }
          h[nt][i] = ok ? hv : 0.0f;
          if (ok) {
            const int64_t bt = (int64_t)(srow + i) * T + t;
            h_out[bt * H + c] = hv;
            gates[bt * H3 + c] = f2bf_u16(r);
            gates[bt * H3 + H + c] = f2bf_u16(z);
            gates[bt * H3 + 2 * H + c] = f2bf_u16(n);
          }
        }
      }
    }
    if (t + 1 < T) {
#pragma unroll
      for (int nt = 0; nt < TILE_NT; ++nt) {
        if (nt < NT) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < 3; ++g) xc[g][nt][i] = xn[g][nt][i];
        }
      }
    }
  }
}

template <bool AUGRU>
__global__ __launch_bounds__(256) void k_gru_tile_bwd(
    const float* __restrict__ dh_out,   // [B,T,H] incoming per-step grads
    const float* __restrict__ h_out,    // [B,T,H] saved states
    const short* __restrict__ gates,    // [B,T,3H] bf16 (r,z,n)
    const short* __restrict__ U, const float* __restrict__ bh,
    const float* __restrict__ alpha, int B, int T, int H,
    short* __restrict__ dpre_x,         // [B,T,3H] bf16
    short* __restrict__ dpre_h,         // [B,T,3H] bf16 (n-part *= r)
    float* __restrict__ dalpha) {       // [B,T] | null
  // pn = h_prev U_n^T: wn_l[n][k] = U[2H + n][k], as the forward's image.
  // carry = dpre_h U sums over the gate row g: ut_l[gate][j][k] =
  // U[gate*H + k][j], the transposed image, so that lane (c, q) again
  // reads B[k = 8q..][col j = c] as 16 B of one row.
  __shared__ __attribute__((aligned(16))) short wn_l[TILE_MAXH][TILE_LD];
  __shared__ __attribute__((aligned(16))) short
      ut_l[3][TILE_MAXH][TILE_LD];
  __shared__ __attribute__((aligned(16))) short
      a_l[4][BWD_TERMS * TILE_PLANE];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int H3 = 3 * H;
  const int NT = (H + 15) >> 4;
  const int KS = (H + 31) >> 5;
  for (int i = threadIdx.x; i < TILE_MAXH * TILE_LD; i += blockDim.x) {
    const int k = i % TILE_LD;
    const int n = i / TILE_LD;
    (&wn_l[0][0])[i] = (n < H && k < H) ? U[(2 * H + n) * H + k] : (short)0;
  }
  for (int i = threadIdx.x; i < 3 * TILE_MAXH * TILE_LD; i += blockDim.x) {
    const int k = i % TILE_LD;
    const int j = (i / TILE_LD) % TILE_MAXH;
    const int g = i / (TILE_LD * TILE_MAXH);
    (&ut_l[0][0][0])[i] = (j < H && k < H) ? U[(g * H + k) * H + j] : (short)0;
  }
  for (int i = lane; i < BWD_TERMS * TILE_PLANE; i += 64) a_l[wave][i] = 0;
  __syncthreads();

  const int col = lane & 15;
  const int row0 = blockIdx.x * TILE_BLOCK_ROWS + wave * TILE_ROWS;
  if (row0 >= B) return;  // no barrier follows
  const int srow = row0 + 4 * (lane >> 4);
  SplitTile<BWD_TERMS> tile(a_l[wave], lane);

  float bias_n[TILE_NT];
#pragma unroll
  for (int nt = 0; nt < TILE_NT; ++nt) {
    const int c = 16 * nt + col;
    bias_n[nt] = c < H ? bh[2 * H + c] : 0.0f;
  }
  f32x4 carry[TILE_NT];  // dh w.r.t. h_t, accumulator layout
#pragma unroll
  for (int nt = 0; nt < TILE_NT; ++nt) carry[nt] = {0.f, 0.f, 0.f, 0.f};

  auto load_h = [&](int t, f32x4 (&hp)[TILE_NT]) {  // h_t, zeros for t < 0
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt) {
      const int c = 16 * nt + col;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = nt < NT && t >= 0 && c < H && srow + i < B;
        hp[nt][i] =
            ok ? h_out[((int64_t)(srow + i) * T + t) * H + c] : 0.0f;
      }
    }
  };
  f32x4 h_prev[TILE_NT], h_next[TILE_NT];
  load_h(T - 2, h_prev);

  for (int t = T - 1; t >= 0; --t) {
    if (t > 0) load_h(t - 2, h_next);
    float a[4];
    if constexpr (AUGRU) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = srow + i < B ? alpha[(int64_t)(srow + i) * T + t] : 0.0f;
    }
    // h_{t-1} -> A operand of pn
    wave_lds_fence();
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt)
      if (nt < NT) tile.put(nt, h_prev[nt]);
    wave_lds_fence();
    bf16x8 af[TILE_KS][BWD_TERMS];
#pragma unroll
    for (int ks = 0; ks < TILE_KS; ++ks)
      if (ks < KS) tile.frags(ks, af[ks]);
    f32x4 dp[3][TILE_NT];  // dpre_h parts, fp32
    float da[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt) {
      if (nt < NT) {
        const float b0 = bias_n[nt];
        f32x4 pn = {b0, b0, b0, b0};
        f32x4 pn_small = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < TILE_KS; ++ks) {
          if (ks < KS) {
            const bf16x8 w =
                lds_frag(&wn_l[16 * nt + col][32 * ks + 8 * (lane >> 4)]);
            mfma_split_apart(af[ks], w, pn, pn_small);
          }
        }
        pn += pn_small;
        const int c = 16 * nt + col;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = c < H && srow + i < B;
          const int64_t bt = (int64_t)(srow + i) * T + t;
          const int64_t gbase = bt * H3 + c;
          float r = 0.0f, z = 0.0f, n = 0.0f, dht = 0.0f;
          if (ok) {
            r = bf2f_u16(gates[gbase]);
            z = bf2f_u16(gates[gbase + H]);
            n = bf2f_u16(gates[gbase + 2 * H]);
            dht = carry[nt][i] + dh_out[bt * H + c];
          }
          const float hp = h_prev[nt][i];
          float eff = 1.0f;
          if constexpr (AUGRU) {
            const float h_cand = (1.0f - z) * n + z * hp;
            da[i] += dht * (h_cand - hp);  // N tiles in ascending order
            eff = a[i];
          }
          const float dn = dht * eff * (1.0f - z);
          const float dz = dht * eff * (hp - n);
          const float direct = dht * ((1.0f - eff) + eff * z);
          const float dpn = dn * (1.0f - n * n);
          const float dpz = dz * z * (1.0f - z);
          const float dr = dpn * pn[i];
          const float dpr = dr * r * (1.0f - r);
          const float dpn_h = dpn * r;
          if (ok) {
            dpre_x[gbase] = f2bf_u16(dpr);
            dpre_x[gbase + H] = f2bf_u16(dpz);
            dpre_x[gbase + 2 * H] = f2bf_u16(dpn);
            dpre_h[gbase] = f2bf_u16(dpr);
            dpre_h[gbase + H] = f2bf_u16(dpz);
            dpre_h[gbase + 2 * H] = f2bf_u16(dpn_h);
          }
          dp[0][nt][i] = ok ? dpr : 0.0f;
          dp[1][nt][i] = ok ? dpz : 0.0f;
          dp[2][nt][i] = ok ? dpn_h : 0.0f;
          carry[nt][i] = ok ? direct : 0.0f;  // seeds the next carry
        }
      }
    }
    if constexpr (AUGRU) {
      // a row's 16 lanes: xor butterfly, the same order whatever the row
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = da[i];
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if (col == 0 && srow + i < B)
          dalpha[(int64_t)(srow + i) * T + t] = v;
      }
    }
    // carry = direct + dpre_h U, one gate (K block) at a time
    f32x4 carry_small[TILE_NT];
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt) carry_small[nt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      wave_lds_fence();
#pragma unroll
      for (int nt = 0; nt < TILE_NT; ++nt)
        if (nt < NT) tile.put(nt, dp[g][nt]);
      wave_lds_fence();
#pragma unroll
      for (int ks = 0; ks < TILE_KS; ++ks)
        if (ks < KS) tile.frags(ks, af[ks]);
#pragma unroll
      for (int nt = 0; nt < TILE_NT; ++nt) {
        if (nt < NT) {
#pragma unroll
          for (int ks = 0; ks < TILE_KS; ++ks) {
            if (ks < KS) {
              const bf16x8 w = lds_frag(
                  &ut_l[g][16 * nt + col][32 * ks + 8 * (lane >> 4)]);
              mfma_split_apart(af[ks], w, carry[nt], carry_small[nt]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int nt = 0; nt < TILE_NT; ++nt) carry[nt] += carry_small[nt];
    if (t > 0) {
#pragma unroll
      for (int nt = 0; nt < TILE_NT; ++nt) h_prev[nt] = h_next[nt];
    }
  }
}

}  // namespace

static void check_gru_tile(int64_t H) {
  TORCH_CHECK(H >= 1 && H <= TILE_MAXH,
              "tile GRU supports hidden size <= 64");
}

std::tuple<torch::Tensor, torch::Tensor> gru_tile_fwd(
    torch::Tensor x3, torch::Tensor u_bf16, torch::Tensor bias_h,
    torch::Tensor alpha, int64_t B, int64_t T, int64_t H) {
  check_gru_tile(H);
  auto h_out = torch::empty({B, T, H},
                            bias_h.options().dtype(torch::kFloat32));
  auto gates = torch::empty({B, T, 3 * H},
                            x3.options().dtype(torch::kBFloat16));
  int blocks = (int)((B + TILE_BLOCK_ROWS - 1) / TILE_BLOCK_ROWS);
  auto stream = current_hip_stream();
  const bool augru = alpha.defined() && alpha.numel() > 0;
  auto* x3p = reinterpret_cast<const short*>(x3.data_ptr<at::BFloat16>());
  auto* up = reinterpret_cast<const short*>(u_bf16.data_ptr<at::BFloat16>());
  auto* gp = reinterpret_cast<short*>(gates.data_ptr<at::BFloat16>());
  if (augru) {
    k_gru_tile_fwd<true><<<blocks, 256, 0, stream>>>(
        x3p, up, bias_h.data_ptr<float>(), alpha.data_ptr<float>(), (int)B,
        (int)T, (int)H, h_out.data_ptr<float>(), gp);
  } else {
    k_gru_tile_fwd<false><<<blocks, 256, 0, stream>>>(
        x3p, up, bias_h.data_ptr<float>(), nullptr, (int)B, (int)T, (int)H,
        h_out.data_ptr<float>(), gp);
  }
  return {h_out, gates};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> gru_tile_bwd(
    torch::Tensor dh_out, torch::Tensor h_out, torch::Tensor gates,
    torch::Tensor u_bf16, torch::Tensor bias_h, torch::Tensor alpha,
    int64_t B, int64_t T, int64_t H) {
  check_gru_tile(H);
  auto dpre_x = torch::empty({B, T, 3 * H},
                             gates.options().dtype(torch::kBFloat16));
  auto dpre_h = torch::empty_like(dpre_x);
  const bool augru = alpha.defined() && alpha.numel() > 0;
  auto dalpha = augru
                    ? torch::empty({B, T},
                                   h_out.options().dtype(torch::kFloat32))
                    : torch::Tensor();
  int blocks = (int)((B + TILE_BLOCK_ROWS - 1) / TILE_BLOCK_ROWS);
  auto stream = current_hip_stream();
  auto* gp = reinterpret_cast<const short*>(gates.data_ptr<at::BFloat16>());
  auto* up = reinterpret_cast<const short*>(u_bf16.data_ptr<at::BFloat16>());
  auto* dxp = reinterpret_cast<short*>(dpre_x.data_ptr<at::BFloat16>());
  auto* dhp = reinterpret_cast<short*>(dpre_h.data_ptr<at::BFloat16>());
  if (augru) {
    k_gru_tile_bwd<true><<<blocks, 256, 0, stream>>>(
        dh_out.contiguous().data_ptr<float>(), h_out.data_ptr<float>(), gp,
        up, bias_h.data_ptr<float>(), alpha.data_ptr<float>(), (int)B,
        (int)T, (int)H, dxp, dhp, dalpha.data_ptr<float>());
  } else {
    k_gru_tile_bwd<false><<<blocks, 256, 0, stream>>>(
        dh_out.contiguous().data_ptr<float>(), h_out.data_ptr<float>(), gp,
        up, bias_h.data_ptr<float>(), nullptr, (int)B, (int)T, (int)H, dxp,
        dhp, nullptr);
  }
  return {dpre_x, dpre_h, dalpha};
}

void register_gru(pybind11::module_& mod) {
  mod.def("gru_fwd", &gru_fwd);
  mod.def("gru_bwd", &gru_bwd);
  mod.def("gru_tile_fwd", &gru_tile_fwd);
  mod.def("gru_tile_bwd", &gru_tile_bwd);
}
