// din_attention_kernels.hip — DIN's local-activation attention as one
// kernel per direction on gfx950 (CDNA4 MFMA). Per sample, over the live
// positions t of mask:
//   f[t]  = bf([s_t, tgt, s_t - tgt, s_t * tgt])   4D wide, as din_feat_fwd
//   h[t]  = sigmoid(f[t] W1^T + b1)                H wide, fp32
//   sc[t] = h[t] . w2                              (b2 cancels in the softmax)
//   w     = softmax over the live t of sc          dead sample: w = 0
//   out   = sum_t w[t] s_t
// The feature rows, h and the scores never reach memory; w is the only
// saved intermediate and backward recomputes f and h from it.
//
// Work split. A workgroup of 4 waves is persistent over samples (grid
// din_attn_grid(B)) and keeps W1 in LDS for its whole life. Within a sample
// wave i takes the 16-position tiles i, i + 4, ...; a tile whose 16 mask
// bytes are all zero is skipped on one ballot.
//
// MFMA formulation. Everything is computed transposed, positions in the
// MFMA column: pre^T[h, t] = W1[h, :] . f[t, :] on v_mfma_f32_16x16x32_bf16
// (A = W1 rows read from LDS, B = the feature fragment built in registers
// from the fp32 seq row and the target). A lane then holds, for its
// position t = lane % 16, the hidden units 16 n + 4 (lane / 16) + i: the
// score is a sum inside the lane and over the four lanes of equal lane % 16,
// and bf(dpre) in this layout IS the B operand (k = 4 (lane / 16) + i) of
// v_mfma_f32_16x16x16_bf16 for
//   df^T[c, t] = sum_h W1[h, c] dpre[t, h]
// whose A operand is W1 read transposed (ds_read_b64_tr_b16) from the same
// LDS copy. Its result gives a lane four consecutive feature columns of its
// position: one 16-B dseq store per (tile, 16 columns).
//   dW1[h, c] = sum_t dpre[t, h] f[t, c]
// needs both operands by columns: each wave stores its tile's f and
// bf(dpre) row-major to LDS, and after a barrier all four waves read the
// four tiles of the round transposed, each wave accumulating the 16-column
// groups c / 16 = wave, wave + 4, ... of dW1 in MFMA accumulators that live
// across all samples of the workgroup (K = the tile's 16 positions: the
// 16x16x16 instruction needs no zero padding). db1 and dw2 accumulate in
// fp32 registers the same way. Each workgroup writes its partials once to
// ws[G, H*4D + 2H]; k_din_attn_merge sums the G partials in ascending
// order: no float atomics, bit-identical from run to run.
// The swizzled LDS tile and the rules of its transposed read: swz_tile.h.

#include "hip_common.h"
#include "mfma_fwd.h"
#include "swz_tile.h"

#include <c10/hip/HIPException.h>

namespace py = pybind11;

namespace {

constexpr int DA_WAVES = 4;
constexpr int DA_THREADS = 64 * DA_WAVES;
constexpr int DA_MAX_D = 64;
constexpr int DA_MAX_H = 128;
constexpr int DA_MAX_T = 1024;
constexpr int DA_MAX_KS = 4 * DA_MAX_D / 32;  // 32-wide K steps of 4D

__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// W1[H, K] bf16 -> LDS tile, columns K .. of the last 64-column tile zero
__device__ __forceinline__ void da_stage_w1(const short* __restrict__ w1,
                                            int H, int K, short* w1s) {
  const int pieces = K >> 3;  // 16-B pieces per row
  for (int i = threadIdx.x; i < H * pieces; i += DA_THREADS) {
    const int row = i / pieces, col = (i - row * pieces) * 8;
    *reinterpret_cast<bf16x8*>(w1s + da_off(H, row, col)) =
        *reinterpret_cast<const bf16x8_u*>(w1 + (int64_t)row * K + col);
  }
  if (K & 63) {  // K % 64 == 32
    const bf16x8 zero = {};
    for (int i = threadIdx.x; i < H * 4; i += DA_THREADS)
      *reinterpret_cast<bf16x8*>(
          w1s + da_off(H, i >> 2, K + (i & 3) * 8)) = zero;
  }
}

// The feature fragments of one 16-position tile: a[s] holds, for position
// lane % 16 (srow: its seq row), feature columns 32 s + 8 (lane / 16) + i.
// D % 8 == 0 keeps the 8 columns inside one of the four segments. One bf16
// rounding of the fp32 value, as k_din_feat_fwd.
template <int KSM>
__device__ __forceinline__ void da_features(const float* __restrict__ srow,
                                            const float* tg, int D, int ks,
                                            int lane, bf16x8 (&a)[KSM]) {
#pragma unroll
  for (int s = 0; s < KSM; ++s) {
    if (s >= ks) break;
    const int c = 32 * s + 8 * (lane >> 4);
    const int seg = (c >= D) + (c >= 2 * D) + (c >= 3 * D);
    const int d0 = c - seg * D;
    const f32x4 s0 = *reinterpret_cast<const f32x4_u*>(srow + d0);
    const f32x4 s1 = *reinterpret_cast<const f32x4_u*>(srow + d0 + 4);
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(tg + d0);
    const f32x4 t1 = *reinterpret_cast<const f32x4*>(tg + d0 + 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float sv = i < 4 ? s0[i] : s1[i - 4];
      const float tv = i < 4 ? t0[i] : t1[i - 4];
      const float v = seg == 0 ? sv
                      : seg == 1 ? tv
                      : seg == 2 ? sv - tv
                                 : sv * tv;
      a[s][i] = f2bf_u16(v);
    }
  }
}

// pre^T of hidden tile n: lane -> position lane % 16, hidden units
// 16 n + 4 (lane / 16) + i; MFMAs in ascending k
template <int KSM>
__device__ __forceinline__ f32x4 da_pre_tile(const short* w1s, int H, int n,
                                             const bf16x8 (&a)[KSM], int ks,
                                             int lane) {
  f32x4 acc = {};
#pragma unroll
  for (int s = 0; s < KSM; ++s) {
    if (s >= ks) break;
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
        w1s + da_off(H, 16 * n + (lane & 15), 32 * s + 8 * (lane >> 4)));
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, a[s], acc, 0, 0, 0);
  }
  return acc;
}

// wave-uniform: does any of the tile's 16 positions live? One ballot.
__device__ __forceinline__ bool da_tile_live(const uint8_t* __restrict__ mk,
                                             int t0, int T, int lane) {
  const int row = t0 + lane;
  const bool lv = lane < 16 && row < T && mk[row] != 0;
  return __ballot(lv) != 0;
}

struct DaShared {  // the part of the LDS carve-up both directions share
  short* w1s;
  float* b1s;
  float* w2s;
  float* tg;   // [64] target row of the sample
  float* red;  // [8] block reductions
  float* pl;   // [4][64] per-wave partial rows
  float* sc;   // [T]
  unsigned char* end;
  __device__ DaShared(unsigned char* base, int H, int K, int T) {
    w1s = reinterpret_cast<short*>(base);
    b1s = reinterpret_cast<float*>(w1s + da_tile_elems(H, K));
    w2s = b1s + H;
    tg = w2s + H;
    red = tg + DA_MAX_D;
    pl = red + 8;
    sc = pl + DA_WAVES * DA_MAX_D;
    end = reinterpret_cast<unsigned char*>(sc + ((T + 3) & ~3));
  }
};

__host__ inline size_t da_shared_bytes(int H, int K, int T) {
  return sizeof(short) * da_tile_elems(H, K) +
         sizeof(float) * (2 * H + DA_MAX_D + 8 + DA_WAVES * DA_MAX_D +
                          ((T + 3) & ~3));
}

__device__ __forceinline__ void da_stage_weights(
    const DaShared& L, const short* __restrict__ w1,
    const float* __restrict__ b1, const short* __restrict__ w2, int H,
    int K) {
  da_stage_w1(w1, H, K, L.w1s);
  for (int i = threadIdx.x; i < H; i += DA_THREADS) {
    L.b1s[i] = b1[i];
    L.w2s[i] = bf2f_u16(w2[i]);
  }
}

// ------------------------------------------------------------------
// Forward. Phase 1: the waves' tiles -> scores in LDS. Phase 2: softmax
// over the live positions (max and sum: wave butterflies, the four waves
// combined in wave order), w to memory, then the pooling: wave p sums
// positions p, p + 4, ... for column lane, the four partial rows are added
// in wave order.
// ------------------------------------------------------------------
__global__ void __launch_bounds__(DA_THREADS) k_din_attn_fwd(
    const float* __restrict__ seq, const float* __restrict__ tgt,
    const uint8_t* __restrict__ mask, const short* __restrict__ w1,
    const float* __restrict__ b1, const short* __restrict__ w2, int B, int T,
    int D, int H, float* __restrict__ out, float* __restrict__ w_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char da_lds[];
  const int K = 4 * D, ks = K / 32, nh = H / 16;
  const DaShared L(da_lds, H, K, T);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g4 = 4 * (lane >> 4);
  da_stage_weights(L, w1, b1, w2, H, K);

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sq = seq + (int64_t)b * T * D;
    const uint8_t* mk = mask + (int64_t)b * T;
    if (tid < D) L.tg[tid] = tgt[(int64_t)b * D + tid];
    __syncthreads();  // tg (and, the first time, the weights) are staged

    for (int t0 = wave * 16; t0 < T; t0 += DA_WAVES * 16) {
      if (!da_tile_live(mk, t0, T, lane)) continue;
      const int row = t0 + (lane & 15);
      bf16x8 a[DA_MAX_KS];
      da_features<DA_MAX_KS>(sq + (int64_t)min(row, T - 1) * D, L.tg, D, ks,
                             lane, a);
      float p = 0.0f;
      for (int n = 0; n < nh; ++n) {
        const f32x4 acc = da_pre_tile<DA_MAX_KS>(L.w1s, H, n, a, ks, lane);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(L.b1s + 16 * n + g4);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(L.w2s + 16 * n + g4);
#pragma unroll
        for (int i = 0; i < 4; ++i) p += da_sigmoid(acc[i] + bv[i]) * wv[i];
      }
      p += __shfl_xor(p, 16, 64);
      p += __shfl_xor(p, 32, 64);
      if (lane < 16 && row < T) L.sc[row] = p;
    }
    __syncthreads();

    // every thread owns positions tid, tid + 256, ... through the phase
    float lmax = -INFINITY;
    for (int t = tid; t < T; t += DA_THREADS)
      if (mk[t]) lmax = fmaxf(lmax, L.sc[t]);
    lmax = wave_max64(lmax);
    if (lane == 0) L.red[wave] = lmax;
    __syncthreads();
    const float m = fmaxf(fmaxf(L.red[0], L.red[1]),
                          fmaxf(L.red[2], L.red[3]));
    float lsum = 0.0f;
    for (int t = tid; t < T; t += DA_THREADS) {
      const float e = mk[t] ? __expf(L.sc[t] - m) : 0.0f;
      L.sc[t] = e;
      lsum += e;
    }
    lsum = wave_sum64(lsum);
    if (lane == 0) L.red[4 + wave] = lsum;
    __syncthreads();
    const float sum = ((L.red[4] + L.red[5]) + L.red[6]) + L.red[7];
    const float inv = sum > 0.0f ? 1.0f / sum : 0.0f;
    for (int t = tid; t < T; t += DA_THREADS) {
      const float wv = L.sc[t] * inv;
      L.sc[t] = wv;
      w_out[(int64_t)b * T + t] = wv;
    }
    __syncthreads();

    float acc = 0.0f;
    if (lane < D) {
      for (int t = wave; t < T; t += DA_WAVES) {
        const float wv = L.sc[t];
        if (wv != 0.0f) acc += wv * sq[(int64_t)t * D + lane];
      }
    }
    L.pl[wave * DA_MAX_D + lane] = acc;
    __syncthreads();
    if (tid < D)
      out[(int64_t)b * D + tid] =
          ((L.pl[tid] + L.pl[DA_MAX_D + tid]) + L.pl[2 * DA_MAX_D + tid]) +
          L.pl[3 * DA_MAX_D + tid];
  }
}

// ------------------------------------------------------------------
// Backward. NHM >= H / 16 and CWM >= ceil(4D / 64) bound the register
// arrays: a wave owns the dW1 column groups wave + 4 ci, ci < CWM, for all
// H / 16 row tiles (4 NHM CWM fp32 per lane), and CWM is also the number of
// 16-column tiles of D and half the number of K steps.
// Per sample: dsc in LDS, then rounds of four tiles. In a round wave i
// works on tile 4 r + i: features and bf(dpre) to its LDS slot, df^T and
// the dseq rows, dtgt partials in registers; after the barrier every wave
// adds the round's live slots to its dW1 groups.
// ------------------------------------------------------------------
template <int NHM, int CWM>
__global__ void __launch_bounds__(DA_THREADS, NHM <= 4 ? 2 : 1) k_din_attn_bwd(
    const float* __restrict__ dout, const float* __restrict__ seq,
    const float* __restrict__ tgt, const uint8_t* __restrict__ mask,
    const float* __restrict__ w, const short* __restrict__ w1,
    const float* __restrict__ b1, const short* __restrict__ w2, int B, int T,
    int D, int H, float* __restrict__ dseq, float* __restrict__ dtgt,
    float* __restrict__ ws) {
  constexpr int KSM = 2 * CWM;
  extern __shared__ __attribute__((aligned(16))) unsigned char da_lds[];
  const int K = 4 * D, ks = K / 32, nh = H / 16, nc = K / 16;
  const int ndt = (D + 15) / 16;
  const DaShared L(da_lds, H, K, T);
  float* dos = reinterpret_cast<float*>(L.end);  // [64] dout row
  int* slot_live = reinterpret_cast<int*>(dos + DA_MAX_D);  // [4]
  short* fts = reinterpret_cast<short*>(slot_live + DA_WAVES);
  const int ft_elems = da_tile_elems(16, K);
  const int dp_elems = da_tile_elems(16, H);
  short* dps = fts + DA_WAVES * ft_elems;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g4 = 4 * (lane >> 4);
  da_stage_weights(L, w1, b1, w2, H, K);

  f32x4 dwacc[NHM][CWM] = {};
  f32x4 db1acc[NHM] = {}, dw2acc[NHM] = {};

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sq = seq + (int64_t)b * T * D;
    const uint8_t* mk = mask + (int64_t)b * T;
    const float* wb = w + (int64_t)b * T;
    float* dsq = dseq + (int64_t)b * T * D;
    if (tid < D) {
      L.tg[tid] = tgt[(int64_t)b * D + tid];
      dos[tid] = dout[(int64_t)b * D + tid];
    }
    __syncthreads();

    // dsc[t] = w[t] (dout . s_t - sum_u w[u] dout . s_u) on live positions
    float lw = 0.0f;
    for (int t = tid; t < T; t += DA_THREADS) {
      float sd = 0.0f;
      if (mk[t]) {
        const float* sp = sq + (int64_t)t * D;
        for (int d = 0; d < D; d += 4) {
          const f32x4 sv = *reinterpret_cast<const f32x4_u*>(sp + d);
          const f32x4 dv = *reinterpret_cast<const f32x4*>(dos + d);
#pragma unroll
          for (int i = 0; i < 4; ++i) sd += dv[i] * sv[i];
        }
        lw += wb[t] * sd;
      }
      L.sc[t] = sd;
    }
    lw = wave_sum64(lw);
    if (lane == 0) L.red[wave] = lw;
    __syncthreads();
    const float wdot = ((L.red[0] + L.red[1]) + L.red[2]) + L.red[3];
    for (int t = tid; t < T; t += DA_THREADS)
      L.sc[t] = mk[t] ? wb[t] * (L.sc[t] - wdot) : 0.0f;
    __syncthreads();

    f32x4 dtacc[CWM] = {};  // dtgt columns 16 dt + g4 + i, this lane's rows
    for (int r0 = 0; r0 < T; r0 += DA_WAVES * 16) {
      const int t0 = r0 + wave * 16;
      const int row = t0 + (lane & 15);
      bool live = false;
      if (t0 < T) live = da_tile_live(mk, t0, T, lane);
      if (t0 < T && !live) {
        // a skipped tile: zero dseq rows, 16 B per lane and step
        const int n4 = min(16, T - t0) * D / 4;
        const f32x4 zero = {};
        for (int i = lane; i < n4; i += 64)
          *reinterpret_cast<f32x4_u*>(dsq + (int64_t)t0 * D + 4 * i) = zero;
      }
      if (live) {  // wave-uniform
        short* ft = fts + wave * ft_elems;
        short* dp = dps + wave * dp_elems;
        const bool row_ok = row < T;
        const int rowc = min(row, T - 1);
        const float* srow = sq + (int64_t)rowc * D;
        const float dsct = row_ok ? L.sc[rowc] : 0.0f;
        const float wt = row_ok ? wb[rowc] : 0.0f;
        bf16x8 a[KSM];
        da_features<KSM>(srow, L.tg, D, ks, lane, a);
#pragma unroll
        for (int s = 0; s < KSM; ++s) {
          if (s >= ks) break;
          *reinterpret_cast<bf16x8*>(
              ft + da_off(16, lane & 15, 32 * s + 8 * (lane >> 4))) = a[s];
        }
        bf16x4 dpk[NHM];
#pragma unroll
        for (int n = 0; n < NHM; ++n) {
          if (n >= nh) break;
          const f32x4 acc = da_pre_tile<KSM>(L.w1s, H, n, a, ks, lane);
          const f32x4 bv =
              *reinterpret_cast<const f32x4*>(L.b1s + 16 * n + g4);
          const f32x4 wv =
              *reinterpret_cast<const f32x4*>(L.w2s + 16 * n + g4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float hv = da_sigmoid(acc[i] + bv[i]);
            // a dead or absent row has dsct == 0: nothing of it is used
            const float dpre =
                dsct != 0.0f ? dsct * wv[i] * hv * (1.0f - hv) : 0.0f;
            db1acc[n][i] += dpre;
            dw2acc[n][i] += dsct != 0.0f ? dsct * hv : 0.0f;
            dpk[n][i] = f2bf_u16(dpre);
          }
          *reinterpret_cast<bf16x4*>(dp + da_off(16, lane & 15,
                                                 16 * n + g4)) = dpk[n];
        }
        // df^T per 16 columns of D and segment; lane: row, columns
        // 16 dt + g4 + i
#pragma unroll
        for (int dt = 0; dt < CWM; ++dt) {
          if (dt >= ndt) break;
          f32x4 df[4] = {};
#pragma unroll
          for (int n = 0; n < NHM; ++n) {
            if (n >= nh) break;
#pragma unroll
            for (int seg = 0; seg < 4; ++seg) {
              // D % 16 == 8: the last tile of a segment runs 8 columns into
              // the next one, or into the zero columns past K; those
              // results belong to no lane with d < D
              const bf16x4 wt4 =
                  da_read_tr(L.w1s, H, 16 * n, seg * D + 16 * dt, lane);
              df[seg] = mfma16(wt4, dpk[n], df[seg]);
            }
          }
          const int d = 16 * dt + g4;
          if (row_ok && d < D) {
            const f32x4 sv = *reinterpret_cast<const f32x4_u*>(srow + d);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(L.tg + d);
            const f32x4 ov = *reinterpret_cast<const f32x4*>(dos + d);
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              o[i] = wt * ov[i] + df[0][i] + df[2][i] + df[3][i] * tv[i];
              if (dsct != 0.0f)
                dtacc[dt][i] += df[1][i] - df[2][i] + df[3][i] * sv[i];
            }
            *reinterpret_cast<f32x4_u*>(dsq + (int64_t)row * D + d) = o;
          }
        }
      }
      if (lane == 0) slot_live[wave] = live ? 1 : 0;
      __syncthreads();

      // dW1[h, c] += sum over the slot's 16 positions of dpre[t, h] f[t, c]
      for (int sl = 0; sl < DA_WAVES; ++sl) {
        if (__builtin_amdgcn_readfirstlane(slot_live[sl]) == 0) continue;
        const short* ft = fts + sl * ft_elems;
        const short* dp = dps + sl * dp_elems;
        bf16x4 fb[CWM];
#pragma unroll
        for (int ci = 0; ci < CWM; ++ci) {
          if (wave + 4 * ci >= nc) break;
          fb[ci] = da_read_tr(ft, 16, 0, 16 * (wave + 4 * ci), lane);
        }
#pragma unroll
        for (int hn = 0; hn < NHM; ++hn) {
          if (hn >= nh) break;
          const bf16x4 da = da_read_tr(dp, 16, 0, 16 * hn, lane);
#pragma unroll
          for (int ci = 0; ci < CWM; ++ci) {
            if (wave + 4 * ci >= nc) break;
            dwacc[hn][ci] = mfma16(da, fb[ci], dwacc[hn][ci]);
          }
        }
      }
      __syncthreads();  // the slots are free for the next round
    }

    // dtgt: the 16 rows of a lane group, then the four waves in order
#pragma unroll
    for (int dt = 0; dt < CWM; ++dt) {
      if (dt >= ndt) break;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = row16_sum(dtacc[dt][i]);
        const int d = 16 * dt + g4 + i;
        if ((lane & 15) == 0 && d < D) L.pl[wave * DA_MAX_D + d] = v;
      }
    }
    __syncthreads();
    if (tid < D)
      dtgt[(int64_t)b * D + tid] =
          ((L.pl[tid] + L.pl[DA_MAX_D + tid]) + L.pl[2 * DA_MAX_D + tid]) +
          L.pl[3 * DA_MAX_D + tid];
    // the next sample's first barrier orders these reads of pl, tg and dos
    // against their next writes: pl is written again only after it
  }

  // this workgroup's partials: [dW1 (H x K) | db1 (H) | dw2 (H)]
  float* wsb = ws + (int64_t)blockIdx.x * ((int64_t)H * K + 2 * H);
#pragma unroll
  for (int hn = 0; hn < NHM; ++hn) {
    if (hn >= nh) break;
#pragma unroll
    for (int ci = 0; ci < CWM; ++ci) {
      const int c = 16 * (wave + 4 * ci) + (lane & 15);
      if (wave + 4 * ci >= nc) break;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        wsb[(int64_t)(16 * hn + g4 + i) * K + c] = dwacc[hn][ci][i];
    }
  }
  // db1 / dw2: the 16 rows of a lane group, then the waves through LDS.
  // No sample is in flight, so the feature slots are free: at least
  // 4 * 16 * 64 shorts, room for [4 waves][2][H <= 128] floats.
  __syncthreads();
  float* part = reinterpret_cast<float*>(fts);
#pragma unroll
  for (int n = 0; n < NHM; ++n) {
    if (n >= nh) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float vb = row16_sum(db1acc[n][i]);
      const float vw = row16_sum(dw2acc[n][i]);
      if ((lane & 15) == 0) {
        part[(wave * 2) * H + 16 * n + g4 + i] = vb;
        part[(wave * 2 + 1) * H + 16 * n + g4 + i] = vw;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * H; i += DA_THREADS)
    wsb[(int64_t)H * K + i] =
        ((part[i] + part[2 * H + i]) + part[4 * H + i]) + part[6 * H + i];
}

// g1[0 .. n1 + H) = sum over the G partials of [dW1 | db1], g2[0 .. H) of
// dw2, in ascending workgroup order; g2[H] = db2 = 0 (the softmax is
// invariant under a shift of the scores).
__global__ void __launch_bounds__(256) k_din_attn_merge(
    const float* __restrict__ ws, int G, int n1, int H,
    float* __restrict__ g1, float* __restrict__ g2) {
  const int n = n1 + 2 * H;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += gridDim.x * blockDim.x) {
    float s = 0.0f;
    for (int g = 0; g < G; ++g) s += ws[(int64_t)g * n + e];
    if (e < n1 + H) g1[e] = s;
    else g2[e - n1 - H] = s;
    if (e == 0) g2[H] = 0.0f;
  }
}

}  // namespace

// ---------------------- host wrappers ----------------------

static size_t din_attn_lds_request(int64_t T, int64_t D, int64_t H, bool bwd) {
  size_t n = da_shared_bytes((int)H, (int)(4 * D), (int)T);
  if (bwd)
    n += sizeof(float) * DA_MAX_D + sizeof(int) * DA_WAVES +
         sizeof(short) * DA_WAVES *
             (da_tile_elems(16, (int)(4 * D)) + da_tile_elems(16, (int)H));
  return n;
}

int64_t din_attn_lds_bytes(int64_t T, int64_t D, int64_t H, bool bwd) {
  return (int64_t)din_attn_lds_request(T, D, H, bwd);
}

// Workgroups either direction launches for B samples: persistent, two per
// compute unit, at most one per sample.
int64_t din_attn_grid(int64_t B) {
  int device = 0, cus = 0;
  C10_HIP_CHECK(hipGetDevice(&device));
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &cus, hipDeviceAttributeMultiprocessorCount, device));
  return std::max<int64_t>(1, std::min<int64_t>(B, 2 * (int64_t)cus));
}

static void check_din_tensor(const char* op, const torch::Tensor& t,
                             const torch::Tensor& like, c10::ScalarType dtype,
                             std::initializer_list<int64_t> shape,
                             const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), op, ": ", name,
              " must be on the GPU of seq");
  TORCH_CHECK(t.scalar_type() == dtype, op, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == c10::IntArrayRef(shape.begin(), shape.size()), op,
              ": ", name, " has shape ", t.sizes(), ", expected ",
              c10::IntArrayRef(shape.begin(), shape.size()));
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

struct DinDims {
  int B, T, D, H;
};

// operands shared by both directions, and the LDS request
static DinDims check_din(const char* op, const torch::Tensor& seq,
                         const torch::Tensor& tgt, const torch::Tensor& mask,
                         const torch::Tensor& w1, const torch::Tensor& b1,
                         const torch::Tensor& w2, bool bwd) {
  TORCH_CHECK(seq.is_cuda() && seq.dim() == 3, op,
              ": seq must be a GPU tensor [B, T, D]");
  TORCH_CHECK(w1.dim() == 2, op, ": w1 must be [H, 4D]");
  const int64_t B = seq.size(0), T = seq.size(1), D = seq.size(2);
  const int64_t H = w1.size(0);
  TORCH_CHECK(D % 8 == 0 && D >= 8 && D <= DA_MAX_D, op,
              ": D must be a multiple of 8 in [8, ", DA_MAX_D, "], got ", D);
  TORCH_CHECK(H % 16 == 0 && H >= 16 && H <= DA_MAX_H, op,
              ": H must be a multiple of 16 in [16, ", DA_MAX_H, "], got ", H);
  TORCH_CHECK(T >= 1 && T <= DA_MAX_T, op, ": T must be in [1, ", DA_MAX_T,
              "], got ", T);
  TORCH_CHECK(B * T * D < (1LL << 31), op, ": B*T*D must stay below 2^31");
  check_din_tensor(op, seq, seq, torch::kFloat32, {B, T, D}, "seq");
  check_din_tensor(op, tgt, seq, torch::kFloat32, {B, D}, "tgt");
  check_din_tensor(op, mask, seq, torch::kUInt8, {B, T}, "mask");
  check_din_tensor(op, w1, seq, torch::kBFloat16, {H, 4 * D}, "w1");
  check_din_tensor(op, b1, seq, torch::kFloat32, {H}, "b1");
  check_din_tensor(op, w2, seq, torch::kBFloat16, {H}, "w2");
  int limit = 0;
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, seq.get_device()));
  const int64_t need = (int64_t)din_attn_lds_request(T, D, H, bwd);
  TORCH_CHECK(need <= limit, op, ": T=", T, " D=", D, " H=", H, " needs ",
              need, " bytes of LDS per block, the device allows ", limit);
  return {(int)B, (int)T, (int)D, (int)H};
}

// A request above the default dynamic-LDS size has to be announced.
template <typename Kern>
static void din_allow_lds(Kern kernel, size_t lds) {
  if (lds > 48 * 1024) {
    C10_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
}

static const short* din_bf_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr<at::BFloat16>());
}

// -> (out f32 [B, D], w f32 [B, T])
std::tuple<torch::Tensor, torch::Tensor> din_attn_fwd(
    torch::Tensor seq, torch::Tensor tgt, torch::Tensor mask,
    torch::Tensor w1, torch::Tensor b1, torch::Tensor w2) {
  const char* op = "din_attn_fwd";
  const DinDims s = check_din(op, seq, tgt, mask, w1, b1, w2, false);
  auto out = torch::empty({s.B, s.D}, seq.options());
  auto w = torch::empty({s.B, s.T}, seq.options());
  if (s.B == 0) return {out, w};
  const size_t lds = din_attn_lds_request(s.T, s.D, s.H, false);
  din_allow_lds(k_din_attn_fwd, lds);
  k_din_attn_fwd<<<(int)din_attn_grid(s.B), DA_THREADS, lds,
                   current_hip_stream()>>>(
      seq.data_ptr<float>(), tgt.data_ptr<float>(), mask.data_ptr<uint8_t>(),
      din_bf_ptr(w1), b1.data_ptr<float>(), din_bf_ptr(w2), s.B, s.T, s.D,
      s.H, out.data_ptr<float>(), w.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {out, w};
}

// -> (dseq [B,T,D], dtgt [B,D], dW1 [H,4D], db1 [H], dw2 [H], db2 [1]), all
// fp32. dw1_out / dw2_out: a layer's flat [dW | db] gradient slice of
// H*4D + H and H + 1 elements; when given it is overwritten in full and the
// weight gradients returned are views of it.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor>
din_attn_bwd(torch::Tensor dout, torch::Tensor seq, torch::Tensor tgt,
             torch::Tensor mask, torch::Tensor w, torch::Tensor w1,
             torch::Tensor b1, torch::Tensor w2,
             c10::optional<torch::Tensor> dw1_out,
             c10::optional<torch::Tensor> dw2_out) {
  const char* op = "din_attn_bwd";
  const DinDims s = check_din(op, seq, tgt, mask, w1, b1, w2, true);
  check_din_tensor(op, dout, seq, torch::kFloat32, {s.B, s.D}, "dout");
  check_din_tensor(op, w, seq, torch::kFloat32, {s.B, s.T}, "w");
  const int64_t n1 = (int64_t)s.H * 4 * s.D;
  auto flat = [&](c10::optional<torch::Tensor>& given, int64_t n,
                  const char* name) {
    if (!given.has_value())
      return torch::empty({n}, seq.options());
    check_din_tensor(op, *given, seq, torch::kFloat32, {n}, name);
    return *given;
  };
  auto g1 = flat(dw1_out, n1 + s.H, "dw1_out");
  auto g2 = flat(dw2_out, s.H + 1, "dw2_out");
  auto dseq = torch::empty_like(seq);
  auto dtgt = torch::empty_like(tgt);
  auto stream = current_hip_stream();
  const int G = s.B == 0 ? 0 : (int)din_attn_grid(s.B);
  auto ws = torch::empty({(int64_t)G, n1 + 2 * s.H}, seq.options());
  if (G > 0) {
    const size_t lds = din_attn_lds_request(s.T, s.D, s.H, true);
#define DIN_ATTN_BWD(NHM, CWM)                                              \
  din_allow_lds(k_din_attn_bwd<NHM, CWM>, lds);                             \
  k_din_attn_bwd<NHM, CWM><<<G, DA_THREADS, lds, stream>>>(                 \
      dout.data_ptr<float>(), seq.data_ptr<float>(), tgt.data_ptr<float>(), \
      mask.data_ptr<uint8_t>(), w.data_ptr<float>(), din_bf_ptr(w1),        \
      b1.data_ptr<float>(), din_bf_ptr(w2), s.B, s.T, s.D, s.H,             \
      dseq.data_ptr<float>(), dtgt.data_ptr<float>(), ws.data_ptr<float>())
    // the register arrays sized for the model's widths, or for the limits
    if (s.H <= 64 && s.D <= 32) {
      DIN_ATTN_BWD(4, 2);
    } else {
      DIN_ATTN_BWD(8, 4);
    }
#undef DIN_ATTN_BWD
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  // G == 0 sums nothing: the gradients are zero
  k_din_attn_merge<<<(int)((n1 + 2 * s.H + 255) / 256), 256, 0, stream>>>(
      ws.data_ptr<float>(), G, (int)n1, s.H, g1.data_ptr<float>(),
      g2.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dseq,
          dtgt,
          g1.narrow(0, 0, n1).view({s.H, 4 * s.D}),
          g1.narrow(0, n1, s.H),
          g2.narrow(0, 0, s.H),
          g2.narrow(0, s.H, 1)};
}

void register_din_attention(py::module_& mod) {
  mod.def("din_attn_fwd", &din_attn_fwd, py::arg("seq"), py::arg("tgt"),
          py::arg("mask"), py::arg("w1"), py::arg("b1"), py::arg("w2"));
  mod.def("din_attn_bwd", &din_attn_bwd, py::arg("dout"), py::arg("seq"),
          py::arg("tgt"), py::arg("mask"), py::arg("w"), py::arg("w1"),
          py::arg("b1"), py::arg("w2"), py::arg("dw1_out") = py::none(),
          py::arg("dw2_out") = py::none());
  mod.def("din_attn_grid", &din_attn_grid, py::arg("B"));
  mod.def("din_attn_lds_bytes", &din_attn_lds_bytes, py::arg("T"),
          py::arg("D"), py::arg("H"), py::arg("bwd"));
}
