// dien_aux_kernels.hip — DIEN's auxiliary next-item loss as one kernel per
// direction on gfx950 (CDNA4 MFMA). For b < B, t < T - 1, flattened to the
// row r = b (T - 1) + t:
//   m    = mask[b,t] mask[b,t+1] (perm[b] != b)
//   x_c  = [bf(h[b,t]) | bf(seq[b,t+1])]      x_n = [bf(h[b,t]) | bf(seq[perm[b],t+1])]
//   a_x  = sigmoid(W1 x + b1)                 A wide, fp32
//   z_x  = a_x . w2 + b2
//   loss = sum m (softplus(-z_c) + softplus(z_n)) / sum m     0 if sum m == 0
// The concatenated rows, a and z never reach memory; forward stores the
// loss and sum m, backward recomputes a and z.
//
// Work split. A workgroup of 4 waves is persistent over rounds of four
// 16-row tiles of r (grid dien_aux_grid(B (T - 1))), wave i on tile
// 4 round + i, and keeps bf(W1) in LDS for its whole life. There is no
// per-sample reduction, so a tile may straddle samples: every lane derives
// b, t and perm[b] of its own row. A tile whose 16 m are all zero is
// skipped on one ballot.
//
// Padded K. The two halves of W1's columns are staged apart, each zero-
// padded to a multiple of 32: padded column c < Hp is h column c, column
// Hp + c is seq column c, K = Hp + Dp <= 128. The x fragments carry zeros
// in the same places, so H = Di = 36 runs on real zeros.
//
// MFMA formulation, transposed as in din_attention_kernels.hip:
// pre^T[a, r] = W1[a, :] . x[r, :] on v_mfma_f32_16x16x32_bf16, A = W1 rows
// from LDS, B = the x fragment built in registers from the fp32 rows.
// P_h = W1[:, :H] bf(h) is computed once per tile and seeds both the click
// and the no-click accumulator: three half-GEMMs, not four. A lane holds,
// for its row lane % 16, the units 16 n + 4 (lane / 16) + i, so z is a sum
// inside the lane and over the four lanes of equal lane % 16, and bf(dpre)
// in this layout is the B operand of v_mfma_f32_16x16x16_bf16 for
//   dx^T[c, r] = sum_a W1[a, c] dpre[r, a]
// whose A operand is W1 read transposed from the same LDS copy; a lane
// gets four consecutive columns of its row: 16-B stores of dh, dclick and
// dnoclick. dW1 is accumulated as in k_din_attn_bwd: every wave stores its
// tile's x = [h | click | noclick] and bf(dpre) = [c | n] row-major to its
// LDS slot; after a barrier all four waves read the round's live slots
// transposed, wave w accumulating the 16-column groups w, w + 4 of dW1 in
// MFMA accumulators that live across all rounds. db1, dw2 and db2
// accumulate in fp32 registers. Each workgroup writes one partial
// [dW1 | db1 | dw2 | db2]; k_dien_aux_merge sums the partials in ascending
// workgroup order: no float atomics, bit-identical from run to run.
//
// Who writes what. The lane of row (b, t) stores dh[b, t], dclick[b, t+1]
// and dnoclick[perm[b], t+1], zeros where m == 0 (dead tiles included);
// the lane of t == T - 2 also zeroes dh[b, T-1], the lane of t == 0 also
// dclick[b, 0] and dnoclick[perm[b], 0]. perm is injective, so every
// element has exactly one writer: no atomics, no pre-fill.

#include "hip_common.h"
#include "mfma_fwd.h"
#include "swz_tile.h"

#include <c10/hip/HIPException.h>

namespace py = pybind11;

namespace {

typedef bf16x4 bf16x4_u __attribute__((aligned(2)));

constexpr int AX_WAVES = 4;
constexpr int AX_THREADS = 64 * AX_WAVES;
constexpr int AX_MAX_W = 64;   // H and Di
constexpr int AX_MAX_A = 128;
constexpr int AX_MAX_CT = AX_MAX_W / 16;  // 16-column tiles of one half

struct AxDims {
  int B, T, H, Di, A;
  __host__ __device__ int Hp() const { return (H + 31) & ~31; }
  __host__ __device__ int Dp() const { return (Di + 31) & ~31; }
  __host__ __device__ int K() const { return Hp() + Dp(); }
  __host__ __device__ int Kr() const { return H + Di; }
  __host__ __device__ int R() const { return B * (T - 1); }
  __host__ __device__ int rounds() const {
    return (R() + 16 * AX_WAVES - 1) / (16 * AX_WAVES);
  }
};

// the row a lane works on; rows past R (and tiles past the last) are
// clamped to row 0 and are not valid
struct AxRow {
  int b, t, pb;
  bool valid, m;
};

__device__ __forceinline__ AxRow ax_row(const AxDims& s, int tile,
                                        const uint8_t* __restrict__ mask,
                                        const int64_t* __restrict__ perm,
                                        int lane) {
  const int r = tile * 16 + (lane & 15);
  AxRow q;
  q.valid = r < s.R();
  const int rc = q.valid ? r : 0;
  q.b = rc / (s.T - 1);
  q.t = rc - q.b * (s.T - 1);
  const int64_t p = perm[q.b];
  q.pb = (int)min(max(p, (int64_t)0), (int64_t)s.B - 1);
  const uint8_t* mk = mask + (int64_t)q.b * s.T + q.t;
  q.m = q.valid && mk[0] != 0 && mk[1] != 0 && p != q.b;
  return q;
}

// bf(W1)[A, H + Di] -> the padded LDS tile; b1 and w2 as fp32
__device__ __forceinline__ void ax_stage(const AxDims& s,
                                         const short* __restrict__ w1,
                                         const float* __restrict__ b1,
                                         const short* __restrict__ w2,
                                         short* w1s, float* b1s, float* w2s) {
  const int Hp = s.Hp();
  const int pieces = ((s.K() + 63) & ~63) >> 2;  // 8-B pieces per row
  for (int i = threadIdx.x; i < s.A * pieces; i += AX_THREADS) {
    const int row = i / pieces, c = (i - row * pieces) * 4;
    const bool ok = c < Hp ? c < s.H : c - Hp < s.Di;
    const int src = c < Hp ? c : s.H + c - Hp;
    bf16x4 v = {};
    if (ok)
      v = *reinterpret_cast<const bf16x4_u*>(w1 + (int64_t)row * s.Kr() + src);
    *reinterpret_cast<bf16x4*>(w1s + da_off(s.A, row, c)) = v;
  }
  for (int i = threadIdx.x; i < s.A; i += AX_THREADS) {
    b1s[i] = b1[i];
    w2s[i] = bf2f_u16(w2[i]);
  }
}

// The fragments of one W-wide fp32 row (W % 4 == 0, W >= 4): x[s] holds the
// padded columns 32 s + 8 (lane / 16) + i, zeros past W and when !keep.
__device__ __forceinline__ void ax_load_x(const float* __restrict__ row, int W,
                                          int ks, bool keep, int lane,
                                          bf16x8 (&x)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    x[s] = bf16x8{};
    if (s >= ks) break;
    const int c = 32 * s + 8 * (lane >> 4);
    const bool ok0 = c < W, ok1 = c + 4 < W;
    const f32x4 v0 = *reinterpret_cast<const f32x4_u*>(row + (ok0 ? c : 0));
    const f32x4 v1 =
        *reinterpret_cast<const f32x4_u*>(row + (ok1 ? c + 4 : 0));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[s][i] = keep && ok0 ? f2bf_u16(v0[i]) : (short)0;
      x[s][4 + i] = keep && ok1 ? f2bf_u16(v1[i]) : (short)0;
    }
  }
}

struct AxFrags {  // one tile's operand rows
  bf16x8 h[2], c[2], n[2];
};

__device__ __forceinline__ void ax_load_rows(const AxDims& s, const AxRow& q,
                                             const float* __restrict__ h,
                                             const float* __restrict__ seq,
                                             bool keep, int lane, AxFrags& x) {
  ax_load_x(h + ((int64_t)q.b * s.T + q.t) * s.H, s.H, s.Hp() / 32, keep,
            lane, x.h);
  ax_load_x(seq + ((int64_t)q.b * s.T + q.t + 1) * s.Di, s.Di, s.Dp() / 32,
            keep, lane, x.c);
  ax_load_x(seq + ((int64_t)q.pb * s.T + q.t + 1) * s.Di, s.Di, s.Dp() / 32,
            keep, lane, x.n);
}

// a_c and a_n of unit tile n: lane -> row lane % 16, units
// 16 n + 4 (lane / 16) + i; MFMAs in ascending k, the h half first
__device__ __forceinline__ void ax_hidden(const AxDims& s, const short* w1s,
                                          const float* b1s, int n,
                                          const AxFrags& x, int lane,
                                          f32x4& ac, f32x4& an) {
  const int row = 16 * n + (lane & 15), kc = 8 * (lane >> 4);
  const int Hp = s.Hp(), ksh = Hp / 32, ksd = s.Dp() / 32;
  f32x4 ph = {};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k >= ksh) break;
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
        w1s + da_off(s.A, row, 32 * k + kc));
    ph = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, x.h[k], ph, 0, 0, 0);
  }
  ac = ph;
  an = ph;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k >= ksd) break;
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
        w1s + da_off(s.A, row, Hp + 32 * k + kc));
    ac = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, x.c[k], ac, 0, 0, 0);
    an = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, x.n[k], an, 0, 0, 0);
  }
  const f32x4 bv =
      *reinterpret_cast<const f32x4*>(b1s + 16 * n + 4 * (lane >> 4));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ac[i] = da_sigmoid(ac[i] + bv[i]);
    an[i] = da_sigmoid(an[i] + bv[i]);
  }
}

// sum over the four lanes of equal lane % 16
__device__ __forceinline__ float col4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// as k_bce_logits_mean_fwd
__device__ __forceinline__ float ax_softplus(float v) {
  return fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v)));
}

struct AxShared {  // the part of the LDS carve-up both directions share
  short* w1s;
  float* b1s;
  float* w2s;
  float* red;  // [8] block reductions
  unsigned char* end;
  __device__ AxShared(unsigned char* base, const AxDims& s) {
    w1s = reinterpret_cast<short*>(base);
    b1s = reinterpret_cast<float*>(w1s + da_tile_elems(s.A, s.K()));
    w2s = b1s + s.A;
    red = w2s + s.A;
    end = reinterpret_cast<unsigned char*>(red + 8);
  }
};

__host__ inline size_t ax_shared_bytes(const AxDims& s) {
  return sizeof(short) * da_tile_elems(s.A, s.K()) +
         sizeof(float) * (2 * s.A + 8);
}

// ------------------------------------------------------------------
// Forward: every workgroup writes part[2 g] = its sum of m (softplus(-z_c)
// + softplus(z_n)) and part[2 g + 1] = its sum of m, both summed over the
// 16 rows of a tile by a wave butterfly and over the waves in wave order.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(AX_THREADS) k_dien_aux_fwd(
    const float* __restrict__ h, const float* __restrict__ seq,
    const uint8_t* __restrict__ mask, const int64_t* __restrict__ perm,
    const short* __restrict__ w1, const float* __restrict__ b1,
    const short* __restrict__ w2, const float* __restrict__ b2, AxDims s,
    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ax_lds[];
  const AxShared L(ax_lds, s);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g4 = 4 * (lane >> 4), nA = s.A / 16;
  ax_stage(s, w1, b1, w2, L.w1s, L.b1s, L.w2s);
  __syncthreads();
  const float bias2 = b2[0];

  float lsum = 0.0f, msum = 0.0f;
  for (int round = blockIdx.x; round < s.rounds(); round += gridDim.x) {
    const AxRow q = ax_row(s, round * AX_WAVES + wave, mask, perm, lane);
    if (__ballot(q.m) == 0) continue;
    AxFrags x;
    ax_load_rows(s, q, h, seq, true, lane, x);
    float zc = 0.0f, zn = 0.0f;
    for (int n = 0; n < nA; ++n) {
      f32x4 ac, an;
      ax_hidden(s, L.w1s, L.b1s, n, x, lane, ac, an);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(L.w2s + 16 * n + g4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        zc += ac[i] * wv[i];
        zn += an[i] * wv[i];
      }
    }
    zc = col4_sum(zc) + bias2;
    zn = col4_sum(zn) + bias2;
    if (q.m && lane < 16) {
      lsum += ax_softplus(-zc) + ax_softplus(zn);
      msum += 1.0f;
    }
  }
  lsum = wave_sum64(lsum);
  msum = wave_sum64(msum);
  if (lane == 0) {
    L.red[wave] = lsum;
    L.red[4 + wave] = msum;
  }
  __syncthreads();
  if (tid == 0) {
    part[2 * blockIdx.x] = ((L.red[0] + L.red[1]) + L.red[2]) + L.red[3];
    part[2 * blockIdx.x + 1] = ((L.red[4] + L.red[5]) + L.red[6]) + L.red[7];
  }
}

// loss = sum of the G loss partials / sum of the G m partials, both in
// ascending workgroup order; exactly 0 when no pair is live (and when G == 0)
__global__ void k_dien_aux_finish(const float* __restrict__ part, int G,
                                  float* __restrict__ loss,
                                  float* __restrict__ msum) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float ls = 0.0f, ms = 0.0f;
  for (int g = 0; g < G; ++g) {
    ls += part[2 * g];
    ms += part[2 * g + 1];
  }
  loss[0] = ms > 0.0f ? ls / ms : 0.0f;
  msum[0] = ms;
}

// ------------------------------------------------------------------
// Backward. NAM >= A / 16 and CWM >= ceil(K / 64) bound the register
// arrays: a wave owns the dW1 column groups wave + 4 ci, ci < CWM, for all
// A / 16 row tiles (4 NAM CWM fp32 per lane).
// Per round wave i works on tile 4 round + i: x and bf(dpre) to its LDS
// slot, dx^T and the rows of dh, dclick and dnoclick (zeros from a dead
// tile); after the barrier every wave adds the round's live slots to its
// dW1 groups.
// ------------------------------------------------------------------
template <int NAM, int CWM>
__global__ void __launch_bounds__(AX_THREADS, NAM <= 4 ? 2 : 1) k_dien_aux_bwd(
    const float* __restrict__ grad_out, const float* __restrict__ msum,
    const float* __restrict__ h, const float* __restrict__ seq,
    const uint8_t* __restrict__ mask, const int64_t* __restrict__ perm,
    const short* __restrict__ w1, const float* __restrict__ b1,
    const short* __restrict__ w2, const float* __restrict__ b2, AxDims s,
    float* __restrict__ dh, float* __restrict__ dclick,
    float* __restrict__ dnoclick, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ax_lds[];
  const AxShared L(ax_lds, s);
  const int Hp = s.Hp(), Dp = s.Dp(), K = s.K(), nA = s.A / 16, nc = K / 16;
  int* slot_live = reinterpret_cast<int*>(L.end);  // [4]
  short* xts = reinterpret_cast<short*>(slot_live + AX_WAVES);
  const int xt_elems = da_tile_elems(16, Hp + 2 * Dp);
  const int dp_elems = da_tile_elems(16, 2 * s.A);
  short* dps = xts + AX_WAVES * xt_elems;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g4 = 4 * (lane >> 4);
  ax_stage(s, w1, b1, w2, L.w1s, L.b1s, L.w2s);
  __syncthreads();
  const float bias2 = b2[0];
  const float total = msum[0];
  const float scale = total > 0.0f ? grad_out[0] / total : 0.0f;

  f32x4 dwacc[NAM][CWM] = {};
  f32x4 db1acc[NAM] = {}, dw2acc[NAM] = {};
  float db2acc = 0.0f;

  for (int round = blockIdx.x; round < s.rounds(); round += gridDim.x) {
    const AxRow q = ax_row(s, round * AX_WAVES + wave, mask, perm, lane);
    const bool live = __ballot(q.m) != 0;  // wave-uniform
    bf16x4 dpc[NAM], dpn[NAM];
    if (live) {
      short* xt = xts + wave * xt_elems;
      short* dp = dps + wave * dp_elems;
      // a row with m == 0 contributes dpre == 0; its x is zeroed as well so
      // that nothing it holds meets that zero in a product
      AxFrags x;
      ax_load_rows(s, q, h, seq, q.m, lane, x);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int c = 32 * k + 8 * (lane >> 4);
        if (32 * k < Hp)
          *reinterpret_cast<bf16x8*>(xt + da_off(16, lane & 15, c)) = x.h[k];
        if (32 * k < Dp) {
          *reinterpret_cast<bf16x8*>(xt + da_off(16, lane & 15, Hp + c)) =
              x.c[k];
          *reinterpret_cast<bf16x8*>(
              xt + da_off(16, lane & 15, Hp + Dp + c)) = x.n[k];
        }
      }
      f32x4 ac[NAM], an[NAM];
      float zc = 0.0f, zn = 0.0f;
#pragma unroll
      for (int n = 0; n < NAM; ++n) {
        if (n >= nA) break;
        ax_hidden(s, L.w1s, L.b1s, n, x, lane, ac[n], an[n]);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(L.w2s + 16 * n + g4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          zc += ac[n][i] * wv[i];
          zn += an[n][i] * wv[i];
        }
      }
      zc = col4_sum(zc) + bias2;
      zn = col4_sum(zn) + bias2;
      const float dzc = q.m ? -da_sigmoid(-zc) * scale : 0.0f;
      const float dzn = q.m ? da_sigmoid(zn) * scale : 0.0f;
      if (lane < 16) db2acc += dzc + dzn;
#pragma unroll
      for (int n = 0; n < NAM; ++n) {
        if (n >= nA) break;
        const f32x4 wv = *reinterpret_cast<const f32x4*>(L.w2s + 16 * n + g4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float hc = ac[n][i], hn = an[n][i];
          dpc[n][i] =
              f2bf_u16(q.m ? dzc * wv[i] * hc * (1.0f - hc) : 0.0f);
          dpn[n][i] =
              f2bf_u16(q.m ? dzn * wv[i] * hn * (1.0f - hn) : 0.0f);
          db1acc[n][i] += bf2f_u16(dpc[n][i]) + bf2f_u16(dpn[n][i]);
          dw2acc[n][i] += q.m ? dzc * hc + dzn * hn : 0.0f;
        }
        *reinterpret_cast<bf16x4*>(
            dp + da_off(16, lane & 15, 16 * n + g4)) = dpc[n];
        *reinterpret_cast<bf16x4*>(
            dp + da_off(16, lane & 15, s.A + 16 * n + g4)) = dpn[n];
      }
    }

    // dh^T per 16 columns of H; lane: its row, columns 16 ct + g4 + i
    const f32x4 zero = {};
#pragma unroll
    for (int ct = 0; ct < AX_MAX_CT; ++ct) {
      if (16 * ct >= s.H) break;
      f32x4 d = {};
      if (live) {
#pragma unroll
        for (int n = 0; n < NAM; ++n) {
          if (n >= nA) break;
          const bf16x4 wt = da_read_tr(L.w1s, s.A, 16 * n, 16 * ct, lane);
          d = mfma16(wt, dpc[n], d);
          d = mfma16(wt, dpn[n], d);
        }
      }
      const int c = 16 * ct + g4;
      if (q.valid && c < s.H) {
        float* row = dh + ((int64_t)q.b * s.T + q.t) * s.H + c;
        *reinterpret_cast<f32x4_u*>(row) = d;
        if (q.t == s.T - 2) *reinterpret_cast<f32x4_u*>(row + s.H) = zero;
      }
    }
#pragma unroll
    for (int ct = 0; ct < AX_MAX_CT; ++ct) {
      if (16 * ct >= s.Di) break;
      f32x4 dc = {}, dn = {};
      if (live) {
#pragma unroll
        for (int n = 0; n < NAM; ++n) {
          if (n >= nA) break;
          const bf16x4 wt =
              da_read_tr(L.w1s, s.A, 16 * n, Hp + 16 * ct, lane);
          dc = mfma16(wt, dpc[n], dc);
          dn = mfma16(wt, dpn[n], dn);
        }
      }
      const int c = 16 * ct + g4;
      if (q.valid && c < s.Di) {
        float* rc = dclick + ((int64_t)q.b * s.T + q.t + 1) * s.Di + c;
        float* rn = dnoclick + ((int64_t)q.pb * s.T + q.t + 1) * s.Di + c;
        *reinterpret_cast<f32x4_u*>(rc) = dc;
        *reinterpret_cast<f32x4_u*>(rn) = dn;
        if (q.t == 0) {
          *reinterpret_cast<f32x4_u*>(rc - s.Di) = zero;
          *reinterpret_cast<f32x4_u*>(rn - s.Di) = zero;
        }
      }
    }
    if (lane == 0) slot_live[wave] = live ? 1 : 0;
    __syncthreads();

    // dW1[a, c] += sum over the slot's 16 rows of dpre[r, a] x[r, c]: the h
    // columns take both dpre against the one h tile, the seq columns dpre_c
    // against click and dpre_n against noclick
    for (int sl = 0; sl < AX_WAVES; ++sl) {
      if (__builtin_amdgcn_readfirstlane(slot_live[sl]) == 0) continue;
      const short* xt = xts + sl * xt_elems;
      const short* dp = dps + sl * dp_elems;
      bf16x4 xb[CWM][2];
#pragma unroll
      for (int ci = 0; ci < CWM; ++ci) {
        const int c0 = 16 * (wave + 4 * ci);
        if (c0 >= K) break;
        xb[ci][0] = da_read_tr(xt, 16, 0, c0, lane);
        xb[ci][1] = c0 < Hp ? xb[ci][0] : da_read_tr(xt, 16, 0, c0 + Dp, lane);
      }
#pragma unroll
      for (int hn = 0; hn < NAM; ++hn) {
        if (hn >= nA) break;
        const bf16x4 dc = da_read_tr(dp, 16, 0, 16 * hn, lane);
        const bf16x4 dn = da_read_tr(dp, 16, 0, s.A + 16 * hn, lane);
#pragma unroll
        for (int ci = 0; ci < CWM; ++ci) {
          if (wave + 4 * ci >= nc) break;
          dwacc[hn][ci] = mfma16(dc, xb[ci][0], dwacc[hn][ci]);
          dwacc[hn][ci] = mfma16(dn, xb[ci][1], dwacc[hn][ci]);
        }
      }
    }
    __syncthreads();  // the slots are free for the next round
  }

  // this workgroup's partial: [dW1 (A x (H + Di)) | db1 (A) | dw2 (A) | db2]
  const int Kr = s.Kr();
  const int64_t n1 = (int64_t)s.A * Kr;
  float* wsb = ws + (int64_t)blockIdx.x * (n1 + 2 * s.A + 1);
#pragma unroll
  for (int hn = 0; hn < NAM; ++hn) {
    if (hn >= nA) break;
#pragma unroll
    for (int ci = 0; ci < CWM; ++ci) {
      if (wave + 4 * ci >= nc) break;
      const int c = 16 * (wave + 4 * ci) + (lane & 15);  // padded column
      const bool ok = c < Hp ? c < s.H : c - Hp < s.Di;
      const int cr = c < Hp ? c : s.H + c - Hp;
      if (!ok) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        wsb[(int64_t)(16 * hn + g4 + i) * Kr + cr] = dwacc[hn][ci][i];
    }
  }
  // db1 / dw2: the 16 rows of a lane group, then the waves through LDS. No
  // round is in flight, so the x slots are free: at least 4 * 16 * 128
  // shorts, room for [4 waves][2][A <= 128] floats.
  float* part = reinterpret_cast<float*>(xts);
#pragma unroll
  for (int n = 0; n < NAM; ++n) {
    if (n >= nA) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float vb = row16_sum(db1acc[n][i]);
      const float vw = row16_sum(dw2acc[n][i]);
      if ((lane & 15) == 0) {
        part[(wave * 2) * s.A + 16 * n + g4 + i] = vb;
        part[(wave * 2 + 1) * s.A + 16 * n + g4 + i] = vw;
      }
    }
  }
  db2acc = wave_sum64(db2acc);
  if (lane == 0) L.red[wave] = db2acc;
  __syncthreads();
  for (int i = tid; i < 2 * s.A; i += AX_THREADS)
    wsb[n1 + i] = ((part[i] + part[2 * s.A + i]) + part[4 * s.A + i]) +
                  part[6 * s.A + i];
  if (tid == 0)
    wsb[n1 + 2 * s.A] = ((L.red[0] + L.red[1]) + L.red[2]) + L.red[3];
}

// out[e] = sum over the G partials of element e, in ascending workgroup
// order; zeros when G == 0
__global__ void __launch_bounds__(256) k_dien_aux_merge(
    const float* __restrict__ ws, int G, int n, float* __restrict__ out) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += gridDim.x * blockDim.x) {
    float v = 0.0f;
    for (int g = 0; g < G; ++g) v += ws[(int64_t)g * n + e];
    out[e] = v;
  }
}

}  // namespace

// ---------------------- host wrappers ----------------------

static size_t dien_aux_lds_request(const AxDims& s, bool bwd) {
  size_t n = ax_shared_bytes(s);
  if (bwd)
    n += sizeof(int) * AX_WAVES +
         sizeof(short) * AX_WAVES *
             (da_tile_elems(16, s.Hp() + 2 * s.Dp()) +
              da_tile_elems(16, 2 * s.A));
  return n;
}

// Workgroups either direction launches for `rows` flattened rows
// b (T - 1) + t: persistent, two per compute unit, at most one per round of
// four 16-row tiles.
int64_t dien_aux_grid(int64_t rows) {
  int device = 0, cus = 0;
  C10_HIP_CHECK(hipGetDevice(&device));
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &cus, hipDeviceAttributeMultiprocessorCount, device));
  const int64_t rounds = (rows + 16 * AX_WAVES - 1) / (16 * AX_WAVES);
  return std::max<int64_t>(1, std::min<int64_t>(rounds, 2 * (int64_t)cus));
}

static void check_ax_tensor(const char* op, const torch::Tensor& t,
                            const torch::Tensor& like, c10::ScalarType dtype,
                            std::initializer_list<int64_t> shape,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), op, ": ", name,
              " must be on the GPU of h");
  TORCH_CHECK(t.scalar_type() == dtype, op, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == c10::IntArrayRef(shape.begin(), shape.size()), op,
              ": ", name, " has shape ", t.sizes(), ", expected ",
              c10::IntArrayRef(shape.begin(), shape.size()));
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

// operands shared by both directions, and the LDS request
static AxDims check_ax(const char* op, const torch::Tensor& h,
                       const torch::Tensor& seq, const torch::Tensor& mask,
                       const torch::Tensor& perm, const torch::Tensor& w1,
                       const torch::Tensor& b1, const torch::Tensor& w2,
                       const torch::Tensor& b2, bool bwd) {
  TORCH_CHECK(h.is_cuda() && h.dim() == 3, op,
              ": h must be a GPU tensor [B, T, H]");
  TORCH_CHECK(seq.dim() == 3, op, ": seq must be [B, T, Di]");
  TORCH_CHECK(w1.dim() == 2, op, ": w1 must be [A, H + Di]");
  const int64_t B = h.size(0), T = h.size(1), H = h.size(2);
  const int64_t Di = seq.size(2), A = w1.size(0);
  TORCH_CHECK(H % 4 == 0 && H >= 4 && H <= AX_MAX_W, op,
              ": H must be a multiple of 4 in [4, ", AX_MAX_W, "], got ", H);
  TORCH_CHECK(Di % 4 == 0 && Di >= 4 && Di <= AX_MAX_W, op,
              ": Di must be a multiple of 4 in [4, ", AX_MAX_W, "], got ", Di);
  TORCH_CHECK(A % 16 == 0 && A >= 16 && A <= AX_MAX_A, op,
              ": A must be a multiple of 16 in [16, ", AX_MAX_A, "], got ", A);
  TORCH_CHECK(T >= 2, op, ": T must be at least 2, got ", T);
  TORCH_CHECK(B * T * std::max(H, Di) < (1LL << 31), op,
              ": B*T*max(H, Di) must stay below 2^31");
  check_ax_tensor(op, h, h, torch::kFloat32, {B, T, H}, "h");
  check_ax_tensor(op, seq, h, torch::kFloat32, {B, T, Di}, "seq");
  check_ax_tensor(op, mask, h, torch::kUInt8, {B, T}, "mask");
  check_ax_tensor(op, perm, h, torch::kInt64, {B}, "perm");
  check_ax_tensor(op, w1, h, torch::kBFloat16, {A, H + Di}, "w1");
  check_ax_tensor(op, b1, h, torch::kFloat32, {A}, "b1");
  check_ax_tensor(op, w2, h, torch::kBFloat16, {A}, "w2");
  check_ax_tensor(op, b2, h, torch::kFloat32, {1}, "b2");
  const AxDims s = {(int)B, (int)T, (int)H, (int)Di, (int)A};
  int limit = 0;
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, h.get_device()));
  const int64_t need = (int64_t)dien_aux_lds_request(s, bwd);
  TORCH_CHECK(need <= limit, op, ": H=", H, " Di=", Di, " A=", A, " needs ",
              need, " bytes of LDS per block, the device allows ", limit);
  return s;
}

// A request above the default dynamic-LDS size has to be announced.
template <typename Kern>
static void ax_allow_lds(Kern kernel, size_t lds) {
  if (lds > 48 * 1024) {
    C10_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
}

static const short* ax_bf_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr<at::BFloat16>());
}

// -> (loss f32 [], sum m f32 [1]), both on the device
std::tuple<torch::Tensor, torch::Tensor> dien_aux_fwd(
    torch::Tensor h, torch::Tensor seq, torch::Tensor mask,
    torch::Tensor perm, torch::Tensor w1, torch::Tensor b1, torch::Tensor w2,
    torch::Tensor b2) {
  const char* op = "dien_aux_fwd";
  const AxDims s = check_ax(op, h, seq, mask, perm, w1, b1, w2, b2, false);
  auto loss = torch::empty({}, h.options());
  auto msum = torch::empty({1}, h.options());
  auto stream = current_hip_stream();
  const int G = s.B == 0 ? 0 : (int)dien_aux_grid(s.R());
  auto part = torch::empty({(int64_t)G, 2}, h.options());
  if (G > 0) {
    const size_t lds = dien_aux_lds_request(s, false);
    ax_allow_lds(k_dien_aux_fwd, lds);
    k_dien_aux_fwd<<<G, AX_THREADS, lds, stream>>>(
        h.data_ptr<float>(), seq.data_ptr<float>(), mask.data_ptr<uint8_t>(),
        perm.data_ptr<int64_t>(), ax_bf_ptr(w1), b1.data_ptr<float>(),
        ax_bf_ptr(w2), b2.data_ptr<float>(), s, part.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  k_dien_aux_finish<<<1, 64, 0, stream>>>(part.data_ptr<float>(), G,
                                          loss.data_ptr<float>(),
                                          msum.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {loss, msum};
}

// -> (dh [B,T,H], dclick [B,T,Di], dnoclick [B,T,Di], dW1 [A,H+Di], db1 [A],
// dw2 [A], db2 [1]), all fp32; the gradient of seq is dclick + dnoclick.
// grad_out: the loss's gradient, one fp32 on the device; msum: dien_aux_fwd's.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor>
dien_aux_bwd(torch::Tensor grad_out, torch::Tensor msum, torch::Tensor h,
             torch::Tensor seq, torch::Tensor mask, torch::Tensor perm,
             torch::Tensor w1, torch::Tensor b1, torch::Tensor w2,
             torch::Tensor b2) {
  const char* op = "dien_aux_bwd";
  const AxDims s = check_ax(op, h, seq, mask, perm, w1, b1, w2, b2, true);
  TORCH_CHECK(grad_out.is_cuda() && grad_out.device() == h.device() &&
                  grad_out.numel() == 1 &&
                  grad_out.scalar_type() == torch::kFloat32,
              op, ": grad_out must be one fp32 value on the GPU of h");
  check_ax_tensor(op, msum, h, torch::kFloat32, {1}, "msum");
  const int64_t n1 = (int64_t)s.A * s.Kr(), n = n1 + 2 * s.A + 1;
  auto dh = torch::empty_like(h);
  auto dclick = torch::empty_like(seq);
  auto dnoclick = torch::empty_like(seq);
  auto grads = torch::empty({n}, h.options());
  auto stream = current_hip_stream();
  const int G = s.B == 0 ? 0 : (int)dien_aux_grid(s.R());
  auto ws = torch::empty({(int64_t)G, n}, h.options());
  if (G > 0) {
    const size_t lds = dien_aux_lds_request(s, true);
#define DIEN_AUX_BWD(NAM, CWM)                                               \
  ax_allow_lds(k_dien_aux_bwd<NAM, CWM>, lds);                               \
  k_dien_aux_bwd<NAM, CWM><<<G, AX_THREADS, lds, stream>>>(                  \
      grad_out.data_ptr<float>(), msum.data_ptr<float>(),                    \
      h.data_ptr<float>(), seq.data_ptr<float>(), mask.data_ptr<uint8_t>(),  \
      perm.data_ptr<int64_t>(), ax_bf_ptr(w1), b1.data_ptr<float>(),         \
      ax_bf_ptr(w2), b2.data_ptr<float>(), s, dh.data_ptr<float>(),          \
      dclick.data_ptr<float>(), dnoclick.data_ptr<float>(),                  \
      ws.data_ptr<float>())
    // the register arrays sized for the model's widths, or for the limits
    if (s.A <= 64 && s.K() <= 64) {
      DIEN_AUX_BWD(4, 1);
    } else {
      DIEN_AUX_BWD(8, 2);
    }
#undef DIEN_AUX_BWD
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  k_dien_aux_merge<<<(int)((n + 255) / 256), 256, 0, stream>>>(
      ws.data_ptr<float>(), G, (int)n, grads.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dh,
          dclick,
          dnoclick,
          grads.narrow(0, 0, n1).view({s.A, s.Kr()}),
          grads.narrow(0, n1, s.A),
          grads.narrow(0, n1 + s.A, s.A),
          grads.narrow(0, n1 + 2 * s.A, 1)};
}

void register_dien_aux(py::module_& mod) {
  mod.def("dien_aux_fwd", &dien_aux_fwd, py::arg("h"), py::arg("seq"),
          py::arg("mask"), py::arg("perm"), py::arg("w1"), py::arg("b1"),
          py::arg("w2"), py::arg("b2"));
  mod.def("dien_aux_bwd", &dien_aux_bwd, py::arg("grad_out"),
          py::arg("msum"), py::arg("h"), py::arg("seq"), py::arg("mask"),
          py::arg("perm"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
          py::arg("b2"));
  mod.def("dien_aux_grid", &dien_aux_grid, py::arg("rows"));
}
