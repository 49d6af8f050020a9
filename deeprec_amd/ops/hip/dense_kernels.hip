// dense_kernels.hip — fused MLP linear layers for gfx950 (CDNA4 MFMA).
//
// DLRM-class MLPs are small (N,K ∈ [16, 512], M = batch): the BLAS library
// picks low-occupancy tiles for them (measured 147us for an 8192x512x16
// layer and 54us for K=8192 weight grads at 12% occupancy). These kernels
// are shaped for exactly this regime instead:
//   fwd:  C[M,N]  = act(A[M,K] @ W[N,K]^T + bias)      (torch Linear layout)
//   dX:   dX[M,K] = G[M,N] @ W[N,K]                    (G = grad ⊙ act mask)
//   dW:   dW[N,K] = G^T[N,M] @ A[M,K], split over M chunks with fp32
//         atomic accumulation (plenty of workgroups even for N=K=256),
//         fused column-sum for dbias.
//
// MFMA: v_mfma_f32_16x16x32_bf16 per-wave tiles; fragment layouts per the
// CDNA4 ISA (A: row=lane%16, k=8*(lane/16)+i; B: col=lane%16, same k;
// D: col=lane%16, row=4*(lane/16)+i) — verified on-device against a torch
// fp32 reference (tests/test_gpu_dense.py, asymmetric random inputs).
// Memory strategy per kernel (all measured on the DLRM layer mix):
//   fwd: operands straight from L2 (weights are L2-resident, A rows
//        stream); 64x64 block tiles maximize block count. A K step's
//        fragment loads are branch-free and issued together, the next
//        step's before this step's MFMAs (register double buffer).
//   dX:  W columns are strided -> W tile staged row-major in LDS and read
//        with the transposed LDS read for the wide-N layers
//        (k_linear_dx_lds), direct for narrow ones.
//   dW:  both operands are column reads -> LDS chunks. N >= 64: 64n x 64k
//        tiles staged row-major and read transposed, several M chunks
//        accumulated in registers to bound the fp32 atomic flush volume
//        (k_linear_dw_lds64t). Narrow N: 16n x 64k tiles, padded LDS rows
//        and scalar column reads (k_linear_dw_lds).

#include "hip_common.h"

#include <algorithm>

namespace py = pybind11;

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// activation gradient of one element: g * act'(out), with out the saved
// bf16 activation; act 1=relu, 2=sigmoid. Shared by k_act_bwd and the dX
// epilogues so that the fused and the two-kernel forms agree bit for bit.
__device__ __forceinline__ short act_grad_u16(short g, short o, int act) {
  const float ov = bf2f_u16(o);
  if (act == 1) return ov > 0.0f ? g : (short)0;
  return f2bf_u16(bf2f_u16(g) * ov * (1.0f - ov));
}

// Load an 8-wide bf16 fragment row: src row-major [rows, cols], fragment
// element i = src[r][k0 + i]; ZERO-FILLED outside bounds.
__device__ __forceinline__ bf16x8 load_frag_row(const short* __restrict__ src,
                                                int r, int k0, int rows,
                                                int cols) {
  bf16x8 out;
  if (r < rows && k0 + 7 < cols) {
    const short* p = src + (int64_t)r * cols + k0;
    // 16B vector load
    out = *reinterpret_cast<const bf16x8*>(p);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      short v = 0;
      if (r < rows && k0 + i < cols) v = src[(int64_t)r * cols + k0 + i];
      out[i] = v;
    }
  }
  return out;
}

// Strided fragment: element i = src[k0 + i][c] (column c of row-major src).
__device__ __forceinline__ bf16x8 load_frag_col(const short* __restrict__ src,
                                                int c, int k0, int rows,
                                                int cols) {
  bf16x8 out;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    short v = 0;
    int r = k0 + i;
    if (r < rows && c < cols) v = src[(int64_t)r * cols + c];
    out[i] = v;
  }
  return out;
}

// ------------------------------------------------------------------
// Row-major LDS tile for operands that arrive by rows and are consumed by
// columns (dW's G and A chunks, dX's W superchunk): [rows][64] bf16, 128-B
// rows, no padding. It is filled with one 16-B store per 16-B global load
// and read back with gfx950's transposed read ds_read_b64_tr_b16: per 16-
// lane group the read takes a block of 4 rows x 16 columns, lane 4q+p of
// the group supplies the address of row q, columns 4p..4p+3, and lane i
// receives column i, row q in element q. A 16x16x32 MFMA fragment (k slots
// 8*(lane/16)+i = tile rows r0+8*(lane/16)+i, fragment row/col = tile
// column cb+lane%16) is two such reads: rows +0..+3 and rows +4..+7.
//
// Banks. The transposed read banks by (addr/4) % 64 per 32-lane half. A
// half holds groups g = 2a and 2a+1, i.e. the 8 tile rows r0+16a+8b+4h+q
// (b, q vary) x one 32-B column block: 8 spans of 8 dwords, 64 dwords, so
// it is conflict-free only if the spans tile all 64 banks. With 128-B rows
// the row contributes 32*(row&1) dwords; the 32-B column block cb/16 is
// XORed with sw(row) = bit1(row) | bit3(row)<<1 = (q>>1) | b<<1, so the
// span starts at 32*(q&1) + 8*((cb/16) ^ sw): all eight (q&1, sw) pairs
// differ -> conflict-free. (Unswizzled padded rows cannot do it: any
// stride that is a multiple of 32 B puts rows r and r+8 on the same
// banks, and a 144-B stride is 2-way.) Stores bank by (addr/4) % 32 in
// groups of 8 consecutive lanes, which here are the eight 16-B segments
// of one row: a permutation of 128 contiguous bytes, conflict-free.
//
// Rules of the transposed read: every lane's address 8-byte aligned and
// inside the tile, and EXEC all ones — the gather crosses lanes, so it
// must stay outside lane-divergent control flow (wave-uniform branches
// are fine); ragged edges are zero-padded in the tile, never masked.
// ------------------------------------------------------------------
using bf16x4 = __attribute__((ext_vector_type(4))) short;
constexpr int TRT_COLS = 64;

// element offset of tile[row][col..]; col % 4 == 0 (and % 8 == 0 for the
// 16-B stores), the 4 (8) elements stay inside one 32-B column block
__device__ __forceinline__ int trt_off(int row, int col) {
  const int sw = ((row >> 1) & 1) | ((row >> 2) & 2);
  return row * TRT_COLS + ((((col >> 4) ^ sw) << 4) | (col & 15));
}

// this lane's read offset for the fragment of rows r0.., columns cb..cb+15,
// relative to row r0; r0 % 16 == 0 keeps sw(r0 + row) == sw(row)
__device__ __forceinline__ int trt_lane_off(int lane, int cb) {
  return trt_off(8 * (lane >> 4) + ((lane >> 2) & 3), cb + 4 * (lane & 3));
}

__device__ __forceinline__ bf16x4 lds_read_tr16(const short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

// fragment whose first read is at p (tile + r0 * TRT_COLS + trt_lane_off):
// elements 0..3 from rows +0..+3, 4..7 from rows +4..+7 (same sw: bit 2)
__device__ __forceinline__ bf16x8 trt_frag(const short* p) {
  const bf16x4 lo = lds_read_tr16(p);
  const bf16x4 hi = lds_read_tr16(p + 4 * TRT_COLS);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Filling such a tile with a 256-thread block, 32 rows (a slab) at a time:
// thread -> row tid/8 of each slab, 16-B segment tid%8. The kernels keep
// their own load batching: load() several slabs, then store() them. A
// kernel that uses it is launched with exactly TRT_STAGE_THREADS threads;
// with fewer, slab rows stay unwritten, with more, stores leave the slab.
constexpr int TRT_STAGE_THREADS = 256;
static_assert(TRT_STAGE_THREADS / 8 == 32, "a slab is 32 rows of 8 segments");
struct TrtStager {
  int row, col, off;  // row in the slab, first column, swizzled offset
  __device__ __forceinline__ explicit TrtStager(int tid)
      : row(tid >> 3), col((tid & 7) * 8), off(trt_off(row, col)) {}
  // this thread's 16 B of src[row0 + 32 slab ..][col0 ..], zero-filled
  // outside [rows, cols]
  __device__ __forceinline__ bf16x8 load(const short* __restrict__ src,
                                         int row0, int slab, int col0,
                                         int rows, int cols) const {
    return load_frag_row(src, row0 + slab * 32 + row, col0 + col, rows, cols);
  }
  __device__ __forceinline__ void store(short* tile, int slab,
                                        bf16x8 v) const {
    *reinterpret_cast<bf16x8*>(&tile[slab * 32 * TRT_COLS + off]) = v;
  }
};

// ------------------------------------------------------------------
// Epilogue pieces. They hold per-lane bounds checks, so none of them may
// contain a transposed read.
// ------------------------------------------------------------------

// one forward element: act(acc + bias) rounded to bf16; act 1=relu (written
// as v < 0 -> 0 so that NaN passes through), 2=sigmoid
__device__ __forceinline__ short fwd_act_u16(float acc, float bv, int act) {
  float v = acc + bv;
  if (act == 1 && v < 0.0f) v = 0.0f;
  else if (act == 2) v = 1.0f / (1.0f + __expf(-v));
  return f2bf_u16(v);
}

// dX store of one wave's 16 x 64 accumulator tile at (m0, c0), kt live
// 16-column subtiles: round to bf16, then (prev_out set) the activation
// gradient of the layer below; bounded by M and K.
__device__ __forceinline__ void dx_store_tile(
    const f32x4 (&acc)[4], int lane, int m0, int c0, int kt, int M, int K,
    short* __restrict__ dX, const short* __restrict__ prev_out,
    int prev_act) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= kt) break;
    const int ck = c0 + t * 16 + (lane & 15);
    if (ck >= K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int cm = m0 + (lane >> 4) * 4 + i;
      if (cm >= M) continue;
      short v = f2bf_u16(acc[t][i]);
      if (prev_out)
        v = act_grad_u16(v, prev_out[(int64_t)cm * K + ck], prev_act);
      dX[(int64_t)cm * K + ck] = v;
    }
  }
}

// dW flush of one wave's NT 16 x 16 accumulators, rows n0.., columns
// k0 + 16 t..: fp32 atomic accumulate, bounded by N and K.
template <int NT>
__device__ __forceinline__ void dw_flush(const f32x4 (&acc)[NT], int lane,
                                         int n0, int k0, int N, int K,
                                         float* __restrict__ dW) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ck = k0 + t * 16 + (lane & 15);
    if (ck >= K) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int cn = n0 + (lane >> 4) * 4 + i;
      if (cn >= N) continue;
      atomicAdd(&dW[(int64_t)cn * K + ck], acc[t][i]);
    }
  }
}

// dbias: each lane sums its 8 m slots of column n0 + lane%16 of every G
// fragment (in slot order) ...
__device__ __forceinline__ float dbias_add_frag(float bsum, bf16x8 gfrag) {
#pragma unroll
  for (int i = 0; i < 8; ++i) bsum += bf2f_u16(gfrag[i]);
  return bsum;
}

// ... and at the end the four lanes of a column are reduced within the
// wave, one atomic per column. Call it wave-uniformly.
__device__ __forceinline__ void dbias_reduce_add(float bsum, int lane, int n0,
                                                 int N,
                                                 float* __restrict__ dbias) {
  float v = bsum;
  for (int off = 16; off < 64; off += 16)
    v += __shfl(bsum, (lane & 15) + off);
  const int cn = n0 + (lane & 15);
  if (lane < 16 && cn < N) atomicAdd(&dbias[cn], v);
}

// ------------------------------------------------------------------
// fwd: C[M,N] = act(A[M,K] @ W[N,K]^T + bias); 4 waves/block stacked on M.
// MT = m-subtiles per wave: each wave computes MT*16 rows x 64 cols, so
// one set of 4 B fragments feeds 4*MT MFMAs. MT=1 maximizes block count
// (latency hiding via parallelism); MT=2 halves B-fragment loads per
// MFMA. (A 128-col NT=8 variant measured WORSE — 44us vs 29us on
// 8192x512x480 — fewer blocks cost more than the halved A re-reads.)
//
// K loop (fwd_accumulate). A wave's only latency hiding is its own loads in flight (the
// DLRM layers give a SIMD 0.5 to 4 waves), so the loop is built around
// that: the MT + 4 fragment loads of a 32-wide K step are unconditional
// 16-B loads from addresses that are always inside the operand, issued
// back to back, and the loads of step i+1 are issued before the MFMAs of
// step i (two register buffers, loop unrolled by two so that both are
// statically named). A bounds test around a load would make the compiler
// branch around it and drain vmcnt after it, one L2 round trip per
// fragment. Rows past M or N are instead read from the clamped last row
// and replaced by zeros with a select (never a multiply: the clamp source
// may hold NaN); waves whose 16*MT x 64 tile is interior (EDGE = false)
// skip clamp and select. The K tail (K % 32) is one more step: with
// K % 8 == 0 a lane's fragment is wholly inside or outside K, outside
// lanes read column 0 of their row and are zeroed by the same select;
// otherwise the element-wise load_frag_row. Each accumulator sees the
// same MFMAs in the same ascending-k order whatever the path.
// ------------------------------------------------------------------
template <int MT>
struct FwdStep {  // one K step of a wave's operands
  bf16x8 a[MT];
  bf16x8 b[4];
};

// 16-B fragment load without an alignment promise: W may start at an odd
// bf16 element, and rows are not 16-B aligned when K % 8 != 0
typedef bf16x8 bf16x8_u __attribute__((aligned(2)));

template <int MT, bool EDGE>
__device__ __forceinline__ void fwd_accumulate(const short* __restrict__ A,
                                               const short* __restrict__ W,
                                               int M, int N, int K, int m0,
                                               int n0, int lane,
                                               f32x4 (&acc)[MT][4]) {
  const int kgrp = (lane >> 4) * 8;
  // this lane's fragment rows at column kgrp, clamped into the operand
  const short* ap[MT];
  const short* bp[4];
  bool a_ok[MT], b_ok[4];
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    const int row = m0 + r * 16 + (lane & 15);
    a_ok[r] = !EDGE || row < M;
    ap[r] = A + (int64_t)(EDGE ? min(row, M - 1) : row) * K + kgrp;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = n0 + t * 16 + (lane & 15);
    b_ok[t] = !EDGE || row < N;
    bp[t] = W + (int64_t)(EDGE ? min(row, N - 1) : row) * K + kgrp;
  }
  auto load = [&](FwdStep<MT>& s, int koff) {
#pragma unroll
    for (int r = 0; r < MT; ++r)
      s.a[r] = *reinterpret_cast<const bf16x8_u*>(ap[r] + koff);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      s.b[t] = *reinterpret_cast<const bf16x8_u*>(bp[t] + koff);
    // keep the scheduler from sinking a step's loads below the MFMAs
    // they are meant to overlap, or its selects in between the loads
    __builtin_amdgcn_sched_barrier(0);
  };
  // zero the fragments of rows past M / N and (kin false) columns past K
  auto zero_fill = [&](FwdStep<MT>& s, bool kin) {
    const bf16x8 zero = {};
#pragma unroll
    for (int r = 0; r < MT; ++r) s.a[r] = (a_ok[r] && kin) ? s.a[r] : zero;
#pragma unroll
    for (int t = 0; t < 4; ++t) s.b[t] = (b_ok[t] && kin) ? s.b[t] : zero;
  };
  auto mfma = [&](const FwdStep<MT>& s) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < MT; ++r)
        acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            s.a[r], s.b[t], acc[r][t], 0, 0, 0);
  };
  auto step = [&](FwdStep<MT>& s) {
    if (EDGE) zero_fill(s, true);
    mfma(s);
  };

  const int nfull = K / 32;
  FwdStep<MT> s0, s1;
  if (nfull > 0) {
    load(s0, 0);
    int i = 0;  // s0 holds step i
    for (; i + 2 < nfull; i += 2) {
      load(s1, (i + 1) * 32);
      step(s0);
      load(s0, (i + 2) * 32);
      step(s1);
    }
    if (i + 2 == nfull) {  // two steps left, nothing to prefetch after them
      load(s1, (i + 1) * 32);
      step(s0);
      step(s1);
    } else {
      step(s0);
    }
  }
  const int kt = nfull * 32;
  if (kt == K) return;
  if ((K & 7) == 0) {
    const bool kin = kt + kgrp < K;
    load(s0, kin ? kt : -kgrp);
    zero_fill(s0, kin);
  } else {
#pragma unroll
    for (int r = 0; r < MT; ++r)
      s0.a[r] = load_frag_row(A, m0 + r * 16 + (lane & 15), kt + kgrp, M, K);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      s0.b[t] = load_frag_row(W, n0 + t * 16 + (lane & 15), kt + kgrp, N, K);
  }
  mfma(s0);
}

template <int MT>
__global__ void __launch_bounds__(256) k_linear_fwd_t(const short* __restrict__ A,
                               const short* __restrict__ W,
                               const float* __restrict__ bias, int M, int N,
                               int K, int act, short* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ntiles64 = (N + 63) / 64;
  const int m0 = (blockIdx.x / ntiles64) * 64 * MT + wave * 16 * MT;
  const int n0 = (blockIdx.x % ntiles64) * 64;
  if (m0 >= M) return;
  f32x4 acc[MT][4] = {};
  const int nt = min(4, (N - n0 + 15) / 16);
  if (m0 + 16 * MT <= M && n0 + 64 <= N)  // wave-uniform
    fwd_accumulate<MT, false>(A, W, M, N, K, m0, n0, lane, acc);
  else
    fwd_accumulate<MT, true>(A, W, M, N, K, m0, n0, lane, acc);
  // D: col = lane%16, row = 4*(lane/16) + i. The MFMA output layout
  // writes 32B fragments per instruction; for FULL 16x64 tiles, stage
  // the tile in LDS and flush 128B row bursts (the fragmented stores
  // capped this kernel at ~520 GB/s on an 8 MB output).
  __shared__ short cstage[4][16][72];  // 72 = 64 + 8 (bank de-phase)
  const bool full_tile =
      (MT == 1) && (n0 + 64 <= N) && (m0 + 16 <= M) && ((N & 7) == 0);
  if (full_tile) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cn = t * 16 + (lane & 15);
      const float bv = bias ? bias[n0 + cn] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cstage[wave][(lane >> 4) * 4 + i][cn] =
            fwd_act_u16(acc[0][t][i], bv, act);
      }
    }
    __builtin_amdgcn_s_waitcnt(0);  // LDS writes visible within the wave
    // flush: 8 lanes per row x 8 cols each = one 16B store per lane,
    // two row-groups of 8 -> full 128B bursts per row
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int row = half * 8 + (lane >> 3);
      const int c8 = (lane & 7) * 8;
      bf16x8 vreg;
#pragma unroll
      for (int j = 0; j < 8; ++j) vreg[j] = cstage[wave][row][c8 + j];
      *reinterpret_cast<bf16x8*>(
          C + (int64_t)(m0 + row) * N + n0 + c8) = vreg;
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < MT; ++r) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= nt) break;
      const int cn = n0 + t * 16 + (lane & 15);
      if (cn >= N) continue;
      const float bv = bias ? bias[cn] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int cm = m0 + r * 16 + (lane >> 4) * 4 + i;
        if (cm >= M) continue;
        C[(int64_t)cm * N + cn] = fwd_act_u16(acc[r][t][i], bv, act);
      }
    }
  }
}

// ------------------------------------------------------------------
// dX[M,K] = G[M,N] @ W[N,K]   (GEMM-K = N; B fragment is strided)
// prev_out [M,K] (optional): the saved output of the layer that produced
// this layer's input. When set, the epilogue stores
// act_grad(bf16(acc), prev_out, prev_act) — the next dX/dW's G operand —
// which removes that layer's k_act_bwd pass over dX.
// ------------------------------------------------------------------
__global__ void k_linear_dx(const short* __restrict__ G,
                            const short* __restrict__ W, int M, int N, int K,
                            short* __restrict__ dX,
                            const short* __restrict__ prev_out,
                            int prev_act) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ktiles64 = (K + 63) / 64;
  const int m0 = (blockIdx.x / ktiles64) * 64 + wave * 16;
  const int c0 = (blockIdx.x % ktiles64) * 64;
  if (m0 >= M) return;
  const int row_g = m0 + (lane & 15);
  const int col_w = c0 + (lane & 15);
  const int kgrp = (lane >> 4) * 8;
  f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                  {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int kt = min(4, (K - c0 + 15) / 16);
  for (int n0 = 0; n0 < N; n0 += 32) {
    bf16x8 a = load_frag_row(G, row_g, n0 + kgrp, M, N);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= kt) break;
      bf16x8 b = load_frag_col(W, col_w + t * 16, n0 + kgrp, N, K);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0,
                                                       0);
    }
  }
  dx_store_tile(acc, lane, m0, c0, kt, M, K, dX, prev_out, prev_act);
}

// ------------------------------------------------------------------
// dX via LDS-staged weights: the 64-col variant above builds its B
// fragments from 8 strided global loads each (W columns); for wide N
// that dominates (measured 37.5us on the 8192x512x480 layer). Here
// W[ns..ns+256][c0..c0+64] is staged ROW-MAJOR into an LDS tile (layout
// and bank arithmetic: trt_off above) once per 256-row N superchunk, one
// 16-B store per 16-B global load, and each B fragment (column c, 8
// consecutive n) is two transposed reads. Each wave computes 32 rows x
// 64 cols (8 MFMAs per pair of G fragments).
// ------------------------------------------------------------------
constexpr int DX_NSUP = 256;  // N rows staged per superchunk (32 KB LDS)
// 32-row slabs loaded together before their LDS stores: one slab at a time
// is one L2 round trip per slab; 2 measured 8 % faster per call, 4 another
// 3 % but 88 VGPRs (5 waves) instead of 72 (7 waves)
constexpr int DX_STAGE_BATCH = 2;
__global__ void k_linear_dx_lds(const short* __restrict__ G,
                                const short* __restrict__ W, int M, int N,
                                int K, short* __restrict__ dX,
                                const short* __restrict__ prev_out,
                                int prev_act) {
  __shared__ __attribute__((aligned(16))) short wl[DX_NSUP * TRT_COLS];
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction; say so, so that the m0 >= M skip below
  // is a scalar branch around the transposed reads
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ktiles64 = (K + 63) / 64;
  const int m0 = (blockIdx.x / ktiles64) * 128 + wave * 32;
  const int c0 = (blockIdx.x % ktiles64) * 64;
  const int row_g0 = m0 + (lane & 15);
  const int row_g1 = m0 + 16 + (lane & 15);
  const int kgrp = (lane >> 4) * 8;
  const int kt = min(4, (K - c0 + 15) / 16);
  const TrtStager stg(threadIdx.x);
  int b_off[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) b_off[t] = trt_lane_off(lane, t * 16);
  f32x4 acc[2][4] = {};
  for (int ns = 0; ns < N; ns += DX_NSUP) {
    const int nlen = min(DX_NSUP, N - ns);
    __syncthreads();  // previous superchunk's reads must finish
    {
      // stage W[ns..ns+nlen][c0..c0+64] -> wl[n][c]; rows past N and
      // columns past K are zero-filled by load_frag_row (no memory access),
      // and every row a fragment can touch (up to the next multiple of 32)
      // is rewritten; a batch may run one slab past that, still inside wl
      const int nstg = (nlen + 31) & ~31;
      for (int it0 = 0; it0 * 32 < nstg; it0 += DX_STAGE_BATCH) {
        bf16x8 v[DX_STAGE_BATCH];
#pragma unroll
        for (int j = 0; j < DX_STAGE_BATCH; ++j)
          v[j] = stg.load(W, ns, it0 + j, c0, N, K);
#pragma unroll
        for (int j = 0; j < DX_STAGE_BATCH; ++j) stg.store(wl, it0 + j, v[j]);
      }
    }
    __syncthreads();
    if (m0 >= M) continue;
    for (int n0 = 0; n0 < nlen; n0 += 32) {
      bf16x8 a0 = load_frag_row(G, row_g0, ns + n0 + kgrp, M, N);
      bf16x8 a1 = load_frag_row(G, row_g1, ns + n0 + kgrp, M, N);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t >= kt) break;
        bf16x8 b = trt_frag(&wl[n0 * TRT_COLS + b_off[t]]);
        acc[0][t] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[0][t], 0, 0,
                                                    0);
        acc[1][t] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[1][t], 0, 0,
                                                    0);
      }
    }
  }
  if (m0 >= M) return;
#pragma unroll
  for (int rg = 0; rg < 2; ++rg)
    dx_store_tile(acc[rg], lane, m0 + rg * 16, c0, kt, M, K, dX, prev_out,
                  prev_act);
}

// dW for narrow N (< 64): block = (16-row N tile) x (64-col K group) x
// (128-row M chunk). G[128,16] and A[128,64] chunks are staged with
// coalesced row loads into padded LDS rows; the four waves compute the four
// 16x16 k-subtiles with scalar column reads (16 consecutive bf16 = 32 B per
// row). fp32 atomic accumulate, one flush per chunk; fused dbias.
__global__ void k_linear_dw_lds(const short* __restrict__ G,
                                const short* __restrict__ A, int M, int N,
                                int K, float* __restrict__ dW,
                                float* __restrict__ dbias) {
  constexpr int CH = 128;      // chunk rows
  constexpr int KG = 64;       // K columns per block
  constexpr int APAD = 8;      // LDS row pad (banks)
  __shared__ short a_l[CH][KG + APAD];
  __shared__ short g_l[CH][16 + APAD];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tid = threadIdx.x;
  const int kgroups = (K + KG - 1) / KG;
  const int tiles_n = (N + 15) / 16;
  const int tile_id = blockIdx.x % (tiles_n * kgroups);
  const int chunk = blockIdx.x / (tiles_n * kgroups);
  const int n0 = (tile_id / kgroups) * 16;
  const int k0 = (tile_id % kgroups) * KG;
  const int mbeg = chunk * CH;

  // stage A[mbeg..mbeg+128][k0..k0+64]: 8 lanes x 16B per row, 32 rows/iter
  {
    const int r_in_iter = tid >> 3;        // 0..31
    const int seg = tid & 7;               // 0..7 (16B segments)
    for (int it = 0; it < CH / 32; ++it) {
      int r = it * 32 + r_in_iter;
      int m = mbeg + r;
      bf16x8 v = load_frag_row(A, m, k0 + seg * 8, M, K);
      *reinterpret_cast<bf16x8*>(&a_l[r][seg * 8]) = v;
    }
    // stage G[mbeg..][n0..n0+16]: 2 lanes x 16B per row, 128 rows/iter
    const int r_g = tid >> 1;              // 0..127
    const int seg_g = tid & 1;
    bf16x8 v = load_frag_row(G, mbeg + r_g, n0 + seg_g * 8, M, N);
    *reinterpret_cast<bf16x8*>(&g_l[r_g][seg_g * 8]) = v;
  }
  __syncthreads();

  // wave w computes dW[n0..n0+16][k0+w*16 .. +16]
  const int kw = wave * 16;
  const int col_a = kw + (lane & 15);
  const int col_g = lane & 15;
  const int kgrp = (lane >> 4) * 8;
  f32x4 acc[1] = {};
  float bsum = 0.0f;
  const bool do_bias = (dbias != nullptr) && (k0 == 0) && (wave == 0);
#pragma unroll
  for (int ms = 0; ms < CH; ms += 32) {
    bf16x8 afrag, gfrag;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int m = ms + kgrp + i;
      gfrag[i] = g_l[m][col_g];
      afrag[i] = a_l[m][col_a];
    }
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfrag, afrag, acc[0], 0,
                                                     0, 0);
    if (do_bias) bsum = dbias_add_frag(bsum, gfrag);
  }
  dw_flush<1>(acc, lane, n0, k0 + kw, N, K, dW);
  if (do_bias) dbias_reduce_add(bsum, lane, n0, N, dbias);
}

// dW for N >= 64: block = 64n x 64k x (cpb x 128)m; wave w owns output
// rows n0+16w..+16, all 64 k columns. With 64-wide tiles the A chunk is
// restaged N/64 times instead of N/16 (252 MB -> 63 MB of A traffic on the
// 8192x512x480 layer). (a) Each MFMA fragment comes from two transposed
// LDS reads of row-major G and A chunks (layout and bank arithmetic:
// trt_off above; the chunks are stored as they are loaded, one 16-B store
// per 16-B global load), and (b) each block accumulates `cpb` consecutive
// 128-row M chunks in registers before its single atomic flush. A
// per-chunk atomic flush was the real bound: 64 chunks x N*K fp32 atomics
// = 63 MB of atomic writes on the 8192x512x480 layer (~31 us of 60 us).
// All 128 rows of both tiles are rewritten every chunk (zero-filled past
// M, N and K by load_frag_row), so a ragged chunk never sums a stale row
// of the chunk before it.
// (Issuing the next chunk's global loads before the MFMA loop and storing
// them after it measured no faster — the 8 loads of a chunk are already in
// flight together and the CU's other blocks cover them — at 122 VGPRs
// instead of 70; profiles/PERF_LOG.md.)
__global__ void k_linear_dw_lds64t(const short* __restrict__ G,
                                   const short* __restrict__ A, int M, int N,
                                   int K, int cpb,
                                   float* __restrict__ dW,
                                   float* __restrict__ dbias) {
  constexpr int CH = 128;
  __shared__ __attribute__((aligned(16))) short a_s[CH * TRT_COLS];
  __shared__ __attribute__((aligned(16))) short g_s[CH * TRT_COLS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int kgroups = (K + 63) / 64;
  const int ngroups = (N + 63) / 64;
  const int tile_id = blockIdx.x % (ngroups * kgroups);
  const int chunk0 = (blockIdx.x / (ngroups * kgroups)) * cpb;
  const int n0 = (tile_id / kgroups) * 64;
  const int k0 = (tile_id % kgroups) * 64;
  const TrtStager stg(threadIdx.x);
  const int g_off = trt_lane_off(lane, wave * 16);
  int a_off[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) a_off[t] = trt_lane_off(lane, t * 16);
  f32x4 acc[4] = {};
  float bsum = 0.0f;
  const bool do_bias = (dbias != nullptr) && (k0 == 0);
  for (int c = 0; c < cpb; ++c) {
    const int mbeg = (chunk0 + c) * CH;
    if (mbeg >= M) break;
    if (c > 0) __syncthreads();  // previous chunk's reads must finish
    // coalesced global row loads, all issued before the first LDS store
    bf16x8 va[CH / 32], vg[CH / 32];
#pragma unroll
    for (int it = 0; it < CH / 32; ++it) {
      va[it] = stg.load(A, mbeg, it, k0, M, K);
      vg[it] = stg.load(G, mbeg, it, n0, M, N);
    }
#pragma unroll
    for (int it = 0; it < CH / 32; ++it) {
      stg.store(a_s, it, va[it]);
      stg.store(g_s, it, vg[it]);
    }
    __syncthreads();
#pragma unroll
    for (int ms = 0; ms < CH; ms += 32) {
      bf16x8 gfrag = trt_frag(&g_s[ms * TRT_COLS + g_off]);
      if (do_bias) bsum = dbias_add_frag(bsum, gfrag);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bf16x8 afrag = trt_frag(&a_s[ms * TRT_COLS + a_off[t]]);
        acc[t] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfrag, afrag, acc[t],
                                                    0, 0, 0);
      }
    }
  }
  dw_flush<4>(acc, lane, n0 + wave * 16, k0, N, K, dW);
  if (do_bias) dbias_reduce_add(bsum, lane, n0 + wave * 16, N, dbias);
}

// ------------------------------------------------------------------
// Fused row L2-normalize: y = x / sqrt(max(sum(x^2), eps)); backward
// dx = (dy - y * <y, dy>) * inv_norm. One wave per row, shfl reduction
// (reference capability: FusedL2Normalize[Grad],
// fused_l2_normalize_op.cc:236,493 — CPU AVX there, CDNA4 wave here).
// ------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
  return __shfl(v, 0);
}

__global__ void k_l2norm_fwd(const short* __restrict__ X, int M, int N,
                             float eps, short* __restrict__ Y,
                             float* __restrict__ inv_norms) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const short* x = X + (int64_t)row * N;
  float ss = 0.0f;
  for (int j = lane; j < N; j += 64) {
    float v = bf2f_u16(x[j]);
    ss += v * v;
  }
  float inv = rsqrtf(fmaxf(wave_sum(ss), eps));
  short* y = Y + (int64_t)row * N;
  for (int j = lane; j < N; j += 64)
    y[j] = f2bf_u16(bf2f_u16(x[j]) * inv);
  if (lane == 0) inv_norms[row] = inv;
}

__global__ void k_l2norm_bwd(const short* __restrict__ dY,
                             const short* __restrict__ Y,
                             const float* __restrict__ inv_norms, int M,
                             int N, short* __restrict__ dX) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const short* dy = dY + (int64_t)row * N;
  const short* y = Y + (int64_t)row * N;
  float dot = 0.0f;
  for (int j = lane; j < N; j += 64)
    dot += bf2f_u16(y[j]) * bf2f_u16(dy[j]);
  dot = wave_sum(dot);
  const float inv = inv_norms[row];
  short* dx = dX + (int64_t)row * N;
  for (int j = lane; j < N; j += 64)
    dx[j] = f2bf_u16((bf2f_u16(dy[j]) - bf2f_u16(y[j]) * dot) * inv);
}

// zero-fill (see ev_kernels k_zero_f32: memset nodes don't replay in
// captured graphs). p may be any 4-byte-aligned slice of a flat buffer
// (FlatDenseAdam hands out [dW | db] slices back to back, so a slice
// after an N = 1 layer starts at an odd element): a scalar head of up to
// 3 floats brings the float4 body to 16-byte alignment, a scalar tail
// finishes the slice.
__global__ void k_zero_f32d(float* __restrict__ p, int64_t n) {
  const int64_t to16 =
      (int64_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;
  const int64_t head = to16 < n ? to16 : n;
  const int64_t nbody = (n - head) & ~3LL;
  float* body = p + head;
  int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 4;
  int64_t stride = gridDim.x * (int64_t)blockDim.x * 4;
  for (; i < nbody; i += stride)
    *reinterpret_cast<float4*>(body + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t j = 0; j < head; ++j) p[j] = 0.0f;
    for (int64_t j = head + nbody; j < n; ++j) p[j] = 0.0f;
  }
}

// ---------------------------------------------------------------------
// fused flat dense Adam (≙ reference dense ApplyAdamAsync,
// training_ali_ops_gpu.cu.cc:534, re-designed as ONE kernel over a flat
// parameter buffer): bias-correction from device-resident beta powers
// (capture-safe, no elementwise prelude), optional bf16 shadow emission
// in the same pass (replaces the per-step multi-tensor cast), optional
// gradient scale (folds the data-parallel 1/world averaging into the
// update so the all-reduce needs no separate div).
__global__ void k_dense_adam(float* __restrict__ w,
                             const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v,
                             short* __restrict__ w16,
                             const float* __restrict__ powers, int64_t n,
                             float lr, float beta1, float beta2, float eps,
                             float gscale) {
  const float lr_t = lr * sqrtf(1.0f - powers[1]) / (1.0f - powers[0]);
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    float gi = g[i] * gscale;
    float mn = beta1 * m[i] + (1.0f - beta1) * gi;
    float vn = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    m[i] = mn;
    v[i] = vn;
    float wn = w[i] - lr_t * mn / (sqrtf(vn) + eps);
    w[i] = wn;
    if (w16) w16[i] = f2bf_u16(wn);
  }
}

// ---------------------------------------------------------------------
// fused residual + LayerNorm (transformer sublayer epilogue).
// torch's LN kernels cost ~930 us/step on [B*T, 32] rows (BST profile);
// one THREAD per row with N as a template parameter keeps every row
// array in registers (a runtime-bounded local array spills to scratch —
// measured 175/348 us per call; this form is bandwidth-bound).
// fwd also emits z = x + a (bf16) and per-row (mean, rstd) for backward.
template <int N>
__global__ void k_resln_fwd(const short* __restrict__ x,
                            const short* __restrict__ a,
                            const float* __restrict__ gamma,
                            const float* __restrict__ beta, int64_t M,
                            float eps, short* __restrict__ y,
                            short* __restrict__ z,
                            float* __restrict__ stats) {
  float gm[N], bt[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    gm[j] = gamma[j];
    bt[j] = beta[j];
  }
  int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; r < M; r += stride) {
    const short* xp = x + r * N;
    const short* ap = a + r * N;
    float zv[N];
    float mean = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      zv[j] = bf2f_u16(xp[j]) + bf2f_u16(ap[j]);
      mean += zv[j];
    }
    mean /= N;
    float var = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float d = zv[j] - mean;
      var += d * d;
    }
    float rstd = rsqrtf(var / N + eps);
    short* yp = y + r * N;
    short* zp = z + r * N;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      zp[j] = f2bf_u16(zv[j]);
      yp[j] = f2bf_u16((zv[j] - mean) * rstd * gm[j] + bt[j]);
    }
    stats[r * 2] = mean;
    stats[r * 2 + 1] = rstd;
  }
}

// backward: dz per row (flows to BOTH residual inputs). dgamma/dbeta
// partials accumulate in REGISTERS across this thread's rows; one LDS
// merge + one global atomic per (block, column) at the end.
template <int N>
__global__ void k_resln_bwd(const short* __restrict__ dy,
                            const short* __restrict__ z,
                            const float* __restrict__ stats,
                            const float* __restrict__ gamma, int64_t M,
                            short* __restrict__ dz,
                            float* __restrict__ dgamma,
                            float* __restrict__ dbeta) {
  __shared__ float ldg[N];
  __shared__ float ldb[N];
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    ldg[j] = 0.0f;
    ldb[j] = 0.0f;
  }
  __syncthreads();
  float gm[N], pg[N], pb[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    gm[j] = gamma[j];
    pg[j] = 0.0f;
    pb[j] = 0.0f;
  }
  int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; r < M; r += stride) {
    const short* dyp = dy + r * N;
    const short* zp = z + r * N;
    const float mean = stats[r * 2];
    const float rstd = stats[r * 2 + 1];
    float s1 = 0.0f, s2 = 0.0f;
    float xh[N], g[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      xh[j] = (bf2f_u16(zp[j]) - mean) * rstd;
      g[j] = bf2f_u16(dyp[j]);
      float gg = g[j] * gm[j];
      s1 += gg;
      s2 += gg * xh[j];
      pg[j] += g[j] * xh[j];
      pb[j] += g[j];
    }
    s1 /= N;
    s2 /= N;
    short* dzp = dz + r * N;
#pragma unroll
    for (int j = 0; j < N; ++j)
      dzp[j] = f2bf_u16((g[j] * gm[j] - s1 - xh[j] * s2) * rstd);
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    atomicAdd(&ldg[j], pg[j]);
    atomicAdd(&ldb[j], pb[j]);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    atomicAdd(&dgamma[j], ldg[j]);
    atomicAdd(&dbeta[j], ldb[j]);
  }
}

// activation backward: G = dY * act_grad(out); act 1=relu, 2=sigmoid
__global__ void k_act_bwd(const short* __restrict__ dY,
                          const short* __restrict__ out, int64_t n, int act,
                          short* __restrict__ G) {
  int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 8;
  int64_t stride = gridDim.x * (int64_t)blockDim.x * 8;
  for (; i + 7 < n; i += stride) {
    bf16x8 g = *reinterpret_cast<const bf16x8*>(dY + i);
    bf16x8 o = *reinterpret_cast<const bf16x8*>(out + i);
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = act_grad_u16(g[j], o[j], act);
    *reinterpret_cast<bf16x8*>(G + i) = r;
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t j = n & ~7LL; j < n; ++j)
      G[j] = act_grad_u16(dY[j], out[j], act);
  }
}

// dense-input preparation: fp32 [M,K] -> bf16 [M,KP] with a zero tail
// (KP >= K), one pass in place of a pad kernel plus a cast kernel. One
// thread per group of 8 output columns; NaN maps to the canonical quiet
// NaN like torch's cast (f2bf_u16 alone would carry a low-mantissa NaN
// into infinity).
__global__ void k_pad_cast_bf16(const float* __restrict__ x, int64_t M, int K,
                                int KP, short* __restrict__ y) {
  const int gpr = (KP + 7) / 8;  // groups per row
  const int64_t ngroups = M * gpr;
  int64_t gi = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; gi < ngroups; gi += stride) {
    const int64_t r = gi / gpr;
    const int c0 = (int)(gi % gpr) * 8;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      short b = 0;
      if (c0 + j < K) {
        const float f = x[r * K + c0 + j];
        b = f != f ? (short)0x7fc0 : f2bf_u16(f);
      }
      v[j] = b;
    }
    short* dst = y + r * KP + c0;
    if ((KP & 7) == 0) {
      *reinterpret_cast<bf16x8*>(dst) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j < KP) dst[j] = v[j];
    }
  }
}

// ------------------------------------------------------------------
// DLRM dot interaction: out[b, p] = <feats[b,i,:], feats[b,j,:]> for
// pairs i<j (upper triangle), padded to P_pad columns with zeros.
// Replaces bmm + triu-gather (library strided-batched GEMM of 27x27x16
// per sample ran at ~325us/step + 63us indexing backward).
// One wave per sample: feats row staged in LDS, each lane computes
// ceil(P/64) pairs. (reference capability: _dot_op, modelzoo/dlrm/
// train.py:121-132 and the Op_dot fusion templates)
// ------------------------------------------------------------------
__global__ void k_interact_fwd(const short* __restrict__ feats, int B, int F,
                               int D, int P, int P_pad,
                               short* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  extern __shared__ short lds[];
  short* f = lds + wave * F * D;
  const bool active = b < B;
  if (active) {
    const short* src = feats + (int64_t)b * F * D;
    for (int t = lane; t * 8 < F * D; t += 64) {
      *reinterpret_cast<bf16x8*>(f + t * 8) =
          *reinterpret_cast<const bf16x8*>(src + t * 8);
    }
  }
  __syncthreads();
  if (!active) return;
  short* dst = reinterpret_cast<short*>(out) + (int64_t)b * P_pad;
  for (int p = lane; p < P_pad; p += 64) {
    if (p >= P) {
      dst[p] = 0;
      continue;
    }
    // pair index -> (i, j), i < j
    int i = 0, rem = p, row = F - 1;
    while (rem >= row) {
      rem -= row;
      --row;
      ++i;
    }
    int j = i + 1 + rem;
    float acc = 0.0f;
    const short* fi = f + i * D;
    const short* fj = f + j * D;
    for (int d = 0; d < D; ++d)
      acc += bf2f_u16(fi[d]) * bf2f_u16(fj[d]);
    dst[p] = f2bf_u16(acc);
  }
}

// backward: dfeats[b,i,d] = sum_j!=i g[b, pair(i,j)] * feats[b,j,d]
// Cat-fused variant: takes bot [B, D] and emb [B, Fe, D] separately and
// emits top_in = [bot | pair dots] [B, D + P_pad] directly — removes the
// two torch cats around the interaction (feats assembly + top-MLP input).
__global__ void k_interact_cat_fwd(const short* __restrict__ bot,
                                   const short* __restrict__ emb, int B,
                                   int Fe, int D, int P, int P_pad,
                                   short* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  const int F = Fe + 1;
  extern __shared__ short lds[];
  short* f = lds + wave * F * D;
  const bool active = b < B;
  if (active) {
    const short* bsrc = bot + (int64_t)b * D;
    for (int t = lane; t * 8 < D; t += 64)
      *reinterpret_cast<bf16x8*>(f + t * 8) =
          *reinterpret_cast<const bf16x8*>(bsrc + t * 8);
    const short* esrc = emb + (int64_t)b * Fe * D;
    for (int t = lane; t * 8 < Fe * D; t += 64)
      *reinterpret_cast<bf16x8*>(f + D + t * 8) =
          *reinterpret_cast<const bf16x8*>(esrc + t * 8);
  }
  __syncthreads();
  if (!active) return;
  short* dst = reinterpret_cast<short*>(out) + (int64_t)b * (D + P_pad);
  for (int d = lane; d < D; d += 64) dst[d] = f[d];  // bot passthrough
  dst += D;
  for (int p = lane; p < P_pad; p += 64) {
    if (p >= P) {
      dst[p] = 0;
      continue;
    }
    int i = 0, rem = p, row = F - 1;
    while (rem >= row) {
      rem -= row;
      --row;
      ++i;
    }
    int j = i + 1 + rem;
    float acc = 0.0f;
    const short* fi = f + i * D;
    const short* fj = f + j * D;
    for (int d = 0; d < D; ++d)
      acc += bf2f_u16(fi[d]) * bf2f_u16(fj[d]);
    dst[p] = f2bf_u16(acc);
  }
}

__global__ void k_interact_cat_bwd(const short* __restrict__ grad,
                                   const short* __restrict__ bot,
                                   const short* __restrict__ emb, int B,
                                   int Fe, int D, int P, int P_pad,
                                   short* __restrict__ dbot,
                                   short* __restrict__ demb) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  const int F = Fe + 1;
  extern __shared__ short lds[];
  short* f = lds + wave * (F * D + ((P + 7) & ~7));
  short* g = f + F * D;
  const bool active = b < B;
  if (active) {
    const short* bsrc = bot + (int64_t)b * D;
    for (int t = lane; t * 8 < D; t += 64)
      *reinterpret_cast<bf16x8*>(f + t * 8) =
          *reinterpret_cast<const bf16x8*>(bsrc + t * 8);
    const short* esrc = emb + (int64_t)b * Fe * D;
    for (int t = lane; t * 8 < Fe * D; t += 64)
      *reinterpret_cast<bf16x8*>(f + D + t * 8) =
          *reinterpret_cast<const bf16x8*>(esrc + t * 8);
    const short* gsrc = grad + (int64_t)b * (D + P_pad) + D;
    for (int t = lane; t < P; t += 64) g[t] = gsrc[t];
  }
  __shared__ short plut[40 * 40];
  for (int t = threadIdx.x; t < F * F; t += blockDim.x) {
    int i = t / F, j = t % F;
    int lo = i < j ? i : j, hi = i < j ? j : i;
    plut[t] = (short)(i == j ? -1
                             : lo * F - (lo * (lo + 1)) / 2 + (hi - lo - 1));
  }
  __syncthreads();
  if (!active) return;
  const short* gdirect = grad + (int64_t)b * (D + P_pad);
  short* db = dbot + (int64_t)b * D;
  short* de = demb + (int64_t)b * Fe * D;
  for (int t = lane; t < F * D; t += 64) {
    int i = t / D, d = t % D;
    float acc = 0.0f;
    const short* prow = &plut[i * F];
    const short* fd = f + d;
#pragma unroll 4
    for (int j = 0; j < F; ++j) {
      int p = prow[j];
      if (p < 0) continue;
      acc += bf2f_u16(g[p]) * bf2f_u16(fd[j * D]);
    }
    if (i == 0) {
      // bot row: the direct top-MLP slice adds in
      db[d] = f2bf_u16(acc + bf2f_u16(gdirect[d]));
    } else {
      de[(i - 1) * D + d] = f2bf_u16(acc);
    }
  }
}

__global__ void k_interact_bwd(const short* __restrict__ grad,
                               const short* __restrict__ feats, int B, int F,
                               int D, int P, int P_pad,
                               short* __restrict__ dfeats) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  extern __shared__ short lds[];
  // per-wave scratch: feats (F*D) + grads (P)
  short* f = lds + wave * (F * D + ((P + 7) & ~7));
  short* g = f + F * D;
  const bool active = b < B;
  if (active) {
    const short* fsrc = feats + (int64_t)b * F * D;
    const short* gsrc = grad + (int64_t)b * P_pad;
    for (int t = lane; t * 8 < F * D; t += 64)
      *reinterpret_cast<bf16x8*>(f + t * 8) =
          *reinterpret_cast<const bf16x8*>(fsrc + t * 8);
    for (int t = lane; t < P; t += 64) g[t] = gsrc[t];
  }
  // per-block pair-index LUT: the triangular index arithmetic in the
  // inner loop cost more ALU than the actual FMAs. ALL threads (active or
  // not) fill it and hit both barriers.
  __shared__ short plut[40 * 40];
  for (int t = threadIdx.x; t < F * F; t += blockDim.x) {
    int i = t / F, j = t % F;
    int lo = i < j ? i : j, hi = i < j ? j : i;
    plut[t] = (short)(i == j ? -1
                             : lo * F - (lo * (lo + 1)) / 2 + (hi - lo - 1));
  }
  __syncthreads();
  if (!active) return;
  short* dst = reinterpret_cast<short*>(dfeats) + (int64_t)b * F * D;
  for (int t = lane; t < F * D; t += 64) {
    int i = t / D, d = t % D;
    float acc = 0.0f;
    const short* prow = &plut[i * F];
    const short* fd = f + d;
#pragma unroll 4
    for (int j = 0; j < F; ++j) {
      int p = prow[j];
      if (p < 0) continue;
      acc += bf2f_u16(g[p]) * bf2f_u16(fd[j * D]);
    }
    dst[t] = f2bf_u16(acc);
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

// The kernels index their operands as dense row-major bf16 matrices; a
// strided view or another dtype would be read as if it were one and
// return numbers, so every wrapper rejects them before launching.
static void check_bf16_matrix(const torch::Tensor& t, const char* op,
                              const char* name) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.dim() == 2, op, ": ", name, " must be 2-D, got ", t.dim(),
              "-D");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": ", name,
              " must be bfloat16, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name,
              " must be contiguous (row-major)");
}

torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w_bf16,
                         torch::Tensor bias, int64_t act,
                         int64_t variant) {
  check_bf16_matrix(x, "linear_fwd", "x");
  check_bf16_matrix(w_bf16, "linear_fwd", "w");
  TORCH_CHECK(x.size(1) == w_bf16.size(1), "linear_fwd: x is [M,",
              x.size(1), "] but w is [N,", w_bf16.size(1), "]");
  int M = x.size(0), K = x.size(1), N = w_bf16.size(0);
  TORCH_CHECK(!bias.defined() || bias.numel() == 0 ||
                  (bias.numel() == N && bias.is_contiguous()),
              "linear_fwd: bias must be empty or contiguous [N]");
  TORCH_CHECK(variant >= -1 && variant <= 1, "linear_fwd: variant must be "
              "-1 (automatic), 0 (MT=1) or 1 (MT=2), got ", variant);
  auto out = torch::empty({M, N}, x.options());
  int tiles_n = (N + 63) / 64;
  const float* bp =
      bias.defined() && bias.numel() ? bias.data_ptr<float>() : nullptr;
  if (variant == 1) {
    int blocks = ((M + 127) / 128) * tiles_n;
    k_linear_fwd_t<2><<<blocks, 256, 0, current_hip_stream()>>>(
        bf_ptr(x), bf_ptr(w_bf16), bp, M, N, K, (int)act, bf_ptr_mut(out));
  } else {  // -1, 0: MT=1 measured fastest across the zoo
    int blocks = ((M + 63) / 64) * tiles_n;
    k_linear_fwd_t<1><<<blocks, 256, 0, current_hip_stream()>>>(
        bf_ptr(x), bf_ptr(w_bf16), bp, M, N, K, (int)act, bf_ptr_mut(out));
  }
  return out;
}

// prev_out/prev_act: fuse the previous layer's activation gradient into
// the epilogue — the result equals act_bwd(linear_dx(g, w), prev_out,
// prev_act) bit for bit. prev_act == 0 leaves dX plain.
torch::Tensor linear_dx(torch::Tensor g, torch::Tensor w_bf16,
                        c10::optional<torch::Tensor> prev_out,
                        int64_t prev_act) {
  check_bf16_matrix(g, "linear_dx", "g");
  check_bf16_matrix(w_bf16, "linear_dx", "w");
  TORCH_CHECK(g.size(1) == w_bf16.size(0), "linear_dx: g is [M,", g.size(1),
              "] but w is [", w_bf16.size(0), ",K]");
  int M = g.size(0), N = g.size(1), K = w_bf16.size(1);
  TORCH_CHECK(prev_act >= 0 && prev_act <= 2, "linear_dx: prev_act must be "
              "0 (none), 1 (relu) or 2 (sigmoid), got ", prev_act);
  const short* pp = nullptr;
  if (prev_out.has_value()) {
    check_bf16_matrix(*prev_out, "linear_dx", "prev_out");
    TORCH_CHECK(prev_out->size(0) == M && prev_out->size(1) == K,
                "linear_dx: prev_out is [", prev_out->size(0), ",",
                prev_out->size(1), "] but dX is [", M, ",", K, "]");
    if (prev_act != 0) pp = bf_ptr(*prev_out);
  } else {
    TORCH_CHECK(prev_act == 0, "linear_dx: prev_act without prev_out");
  }
  auto dx = torch::empty({M, K}, g.options());
  int tiles_k = (K + 63) / 64;
  if (N >= 128) {
    // wide GEMM-K: strided W-column loads dominate -> LDS-staged variant
    int blocks = ((M + 127) / 128) * tiles_k;
    k_linear_dx_lds<<<blocks, TRT_STAGE_THREADS, 0, current_hip_stream()>>>(
        bf_ptr(g), bf_ptr(w_bf16), M, N, K, bf_ptr_mut(dx), pp,
        (int)prev_act);
  } else {
    int blocks = ((M + 63) / 64) * tiles_k;
    k_linear_dx<<<blocks, 256, 0, current_hip_stream()>>>(
        bf_ptr(g), bf_ptr(w_bf16), M, N, K, bf_ptr_mut(dx), pp,
        (int)prev_act);
  }
  return dx;
}

static void zero_f32_launch(float* p, int64_t n) {
  k_zero_f32d<<<(int)std::clamp<int64_t>((n / 4 + 255) / 256, 1, 1024), 256,
                0, current_hip_stream()>>>(p, n);
}

// Shared body of linear_dw (ws undefined: allocated here) and linear_dw_out
// (ws = the caller's flat [N*K (+ N)] slice); `op` names the binding in the
// messages. Every check runs before anything is zero-filled or launched.
// zero = false: the caller has cleared ws already (one zero_f32 over a
// whole tower's adjacent slices); the kernels only accumulate.
static std::tuple<torch::Tensor, torch::Tensor> linear_dw_impl(
    const char* op, torch::Tensor g, torch::Tensor x, torch::Tensor ws,
    bool want_bias, int64_t variant, bool zero) {
  check_bf16_matrix(g, op, "g");
  check_bf16_matrix(x, op, "x");
  TORCH_CHECK(g.size(0) == x.size(0), op, ": g has ", g.size(0),
              " rows but x has ", x.size(0));
  TORCH_CHECK(variant == -1 || variant == 0 || variant == 2, op,
              ": variant must be -1 (automatic), 0 (k_linear_dw_lds) or 2 "
              "(k_linear_dw_lds64t), got ", variant);
  int M = g.size(0), N = g.size(1), K = x.size(1);
  int64_t ws_len = (int64_t)N * K + (want_bias ? N : 0);
  if (ws.defined()) {
    TORCH_CHECK(ws.is_cuda() && ws.is_contiguous() &&
                    ws.scalar_type() == torch::kFloat32 &&
                    ws.numel() == ws_len,
                op, ": ws must be a contiguous fp32 GPU tensor of ", ws_len,
                " elements");
  } else {
    ws = torch::empty({ws_len}, g.options().dtype(torch::kFloat32));
  }
  // one fill-kernel zero for dW + dbias (cheaper than torch's fill
  // machinery; hipMemsetAsync is avoided: memset nodes recorded during
  // hipGraph capture were observed not to replay)
  if (zero) zero_f32_launch(ws.data_ptr<float>(), ws_len);
  auto dw = ws.narrow(0, 0, (int64_t)N * K).view({N, K});
  auto db = want_bias ? ws.narrow(0, (int64_t)N * K, N) : torch::Tensor();
  int m_chunks = (M + 127) / 128;
  float* dbp = want_bias ? db.data_ptr<float>() : nullptr;
  if (variant < 0) variant = N >= 64 ? 2 : 0;
  if (variant == 2) {
    // 64-wide tiles, transposed LDS, multi-chunk register accumulation:
    // pick chunks-per-block so the grid stays ~1024 blocks while the
    // atomic flush volume drops by cpb x
    int tiles = ((N + 63) / 64) * ((K + 63) / 64);
    int cpb = std::max(1, (int)((int64_t)m_chunks * tiles / 512));
    int blocks = tiles * ((m_chunks + cpb - 1) / cpb);
    k_linear_dw_lds64t<<<blocks, TRT_STAGE_THREADS, 0,
                         current_hip_stream()>>>(
        bf_ptr(g), bf_ptr(x), M, N, K, cpb, dw.data_ptr<float>(), dbp);
  } else {
    int tiles = ((N + 15) / 16) * ((K + 63) / 64);
    k_linear_dw_lds<<<tiles * m_chunks, 256, 0, current_hip_stream()>>>(
        bf_ptr(g), bf_ptr(x), M, N, K, dw.data_ptr<float>(), dbp);
  }
  return {dw, db};
}

std::tuple<torch::Tensor, torch::Tensor> linear_dw(torch::Tensor g,
                                                   torch::Tensor x,
                                                   bool want_bias,
                                                   int64_t variant) {
  return linear_dw_impl("linear_dw", g, x, torch::Tensor(), want_bias,
                        variant, true);
}

// dW/db written into a caller-provided flat [N*K + N] workspace — a view
// of the optimizer's flat gradient buffer, so backward lands gradients
// exactly where the fused dense Adam reads them (no flatten/unflatten
// copies around the all-reduce).
std::tuple<torch::Tensor, torch::Tensor> linear_dw_out(torch::Tensor g,
                                                       torch::Tensor x,
                                                       torch::Tensor ws,
                                                       bool want_bias,
                                                       int64_t variant,
                                                       bool zero) {
  TORCH_CHECK(ws.defined(), "linear_dw_out: ws is undefined");
  return linear_dw_impl("linear_dw_out", g, x, ws, want_bias, variant, zero);
}

// clear any contiguous fp32 1-D tensor with the capture-safe fill kernel
void zero_f32(torch::Tensor ws) {
  TORCH_CHECK(ws.is_cuda() && ws.dim() == 1 && ws.is_contiguous() &&
                  ws.scalar_type() == torch::kFloat32,
              "zero_f32: ws must be a contiguous 1-D fp32 GPU tensor");
  if (ws.numel() == 0) return;
  zero_f32_launch(ws.data_ptr<float>(), ws.numel());
}

// x fp32 [M,K] -> bf16 [M,k_pad], columns K.. zero; rounding as torch's
// fp32 -> bf16 cast (nearest even)
torch::Tensor pad_cast_bf16(torch::Tensor x, int64_t k_pad) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat32,
              "pad_cast_bf16: x must be a contiguous 2-D fp32 GPU tensor");
  int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(k_pad >= K, "pad_cast_bf16: k_pad ", k_pad, " < K ", K);
  TORCH_CHECK(k_pad < (1 << 30), "pad_cast_bf16: k_pad ", k_pad,
              " is out of range (< 2^30)");
  auto y = torch::empty({M, k_pad}, x.options().dtype(torch::kBFloat16));
  if (M == 0 || k_pad == 0) return y;
  int64_t groups = M * ((k_pad + 7) / 8);
  int blocks = (int)std::clamp<int64_t>((groups + 255) / 256, 1, 4096);
  k_pad_cast_bf16<<<blocks, 256, 0, current_hip_stream()>>>(
      x.data_ptr<float>(), M, (int)K, (int)k_pad, bf_ptr_mut(y));
  return y;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> resln_fwd(
    torch::Tensor x, torch::Tensor a, torch::Tensor gamma,
    torch::Tensor beta, double eps) {
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous());
  int64_t M = x.numel() / x.size(-1);
  int N = x.size(-1);
  TORCH_CHECK(N <= 64, "resln: row width must be <= 64");
  auto y = torch::empty_like(x);
  auto z = torch::empty_like(x);
  auto stats = torch::empty({M, 2}, x.options().dtype(torch::kFloat32));
  if (M == 0) return {y, z, stats};
  TORCH_CHECK(N == 16 || N == 32 || N == 64, "resln: N must be 16/32/64");
  int blocks = (int)std::min<int64_t>((M + 255) / 256, 4096);
#define RESLN_FWD(NV) \
  k_resln_fwd<NV><<<blocks, 256, 0, current_hip_stream()>>>( \
      bf_ptr(x), bf_ptr(a), gamma.data_ptr<float>(), \
      beta.data_ptr<float>(), M, (float)eps, bf_ptr_mut(y), \
      bf_ptr_mut(z), stats.data_ptr<float>())
  if (N == 16) RESLN_FWD(16);
  else if (N == 32) RESLN_FWD(32);
  else RESLN_FWD(64);
#undef RESLN_FWD
  return {y, z, stats};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> resln_bwd(
    torch::Tensor dy, torch::Tensor z, torch::Tensor stats,
    torch::Tensor gamma) {
  int64_t M = z.numel() / z.size(-1);
  int N = z.size(-1);
  auto dz = torch::empty_like(z);
  auto opts = gamma.options();
  auto dgamma = torch::empty({N}, opts);
  auto dbeta = torch::empty({N}, opts);
  auto stream = current_hip_stream();
  k_zero_f32d<<<1, 64, 0, stream>>>(dgamma.data_ptr<float>(), N);
  k_zero_f32d<<<1, 64, 0, stream>>>(dbeta.data_ptr<float>(), N);
  if (M == 0) return {dz, dgamma, dbeta};
  auto dyc = dy.contiguous();
  // ~8 rows per thread amortize the dgamma/dbeta partial merges
  int blocks = (int)std::min<int64_t>((M + 256 * 8 - 1) / (256 * 8), 4096);
  blocks = std::max(blocks, 64);
#define RESLN_BWD(NV) \
  k_resln_bwd<NV><<<blocks, 256, 0, stream>>>( \
      bf_ptr(dyc), bf_ptr(z), stats.data_ptr<float>(), \
      gamma.data_ptr<float>(), M, bf_ptr_mut(dz), \
      dgamma.data_ptr<float>(), dbeta.data_ptr<float>())
  if (N == 16) RESLN_BWD(16);
  else if (N == 32) RESLN_BWD(32);
  else RESLN_BWD(64);
#undef RESLN_BWD
  return {dz, dgamma, dbeta};
}

void dense_adam(torch::Tensor w, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, torch::Tensor w16, torch::Tensor powers,
                double lr, double beta1, double beta2, double eps,
                double gscale) {
  int64_t n = w.numel();
  if (n == 0) return;
  short* w16p = (w16.defined() && w16.numel())
                    ? reinterpret_cast<short*>(w16.data_ptr<at::BFloat16>())
                    : nullptr;
  int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  k_dense_adam<<<blocks, 256, 0, current_hip_stream()>>>(
      w.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
      v.data_ptr<float>(), w16p, powers.data_ptr<float>(), n, (float)lr,
      (float)beta1, (float)beta2, (float)eps, (float)gscale);
}

torch::Tensor act_bwd(torch::Tensor dy, torch::Tensor out, int64_t act) {
  auto g = torch::empty_like(dy);
  int64_t n = dy.numel();
  int blocks = (int)std::min<int64_t>((n / 8 + 255) / 256, 4096);
  k_act_bwd<<<std::max(blocks, 1), 256, 0, current_hip_stream()>>>(
      bf_ptr(dy), bf_ptr(out), n, (int)act, bf_ptr_mut(g));
  return g;
}

torch::Tensor interact_fwd(torch::Tensor feats, int64_t p_pad) {
  TORCH_CHECK(feats.scalar_type() == torch::kBFloat16 &&
              feats.is_contiguous());
  int B = feats.size(0), F = feats.size(1), D = feats.size(2);
  int P = F * (F - 1) / 2;
  TORCH_CHECK((F * D) % 8 == 0, "F*D must be a multiple of 8");
  auto out = torch::empty({B, p_pad}, feats.options());
  int blocks = (B + 3) / 4;
  size_t lds = 4 * (size_t)F * D * sizeof(short);
  k_interact_fwd<<<blocks, 256, lds, current_hip_stream()>>>(
      bf_ptr(feats), B, F, D, P, (int)p_pad, bf_ptr_mut(out));
  return out;
}

torch::Tensor interact_bwd(torch::Tensor grad, torch::Tensor feats) {
  int B = feats.size(0), F = feats.size(1), D = feats.size(2);
  TORCH_CHECK(F <= 40, "interact_bwd: pair LUT supports F <= 40");
  int P = F * (F - 1) / 2;
  int P_pad = grad.size(1);
  auto dfeats = torch::empty_like(feats);
  int blocks = (B + 3) / 4;
  size_t lds = 4 * (size_t)(F * D + ((P + 7) & ~7)) * sizeof(short);
  k_interact_bwd<<<blocks, 256, lds, current_hip_stream()>>>(
      bf_ptr(grad.contiguous()), bf_ptr(feats), B, F, D, P, P_pad,
      bf_ptr_mut(dfeats));
  return dfeats;
}

torch::Tensor interact_cat_fwd(torch::Tensor bot, torch::Tensor emb,
                               int64_t p_pad) {
  TORCH_CHECK(bot.scalar_type() == torch::kBFloat16 && bot.is_contiguous());
  TORCH_CHECK(emb.scalar_type() == torch::kBFloat16 && emb.is_contiguous());
  int B = emb.size(0), Fe = emb.size(1), D = emb.size(2);
  int F = Fe + 1;
  int P = F * (F - 1) / 2;
  TORCH_CHECK(D % 8 == 0, "D must be a multiple of 8");
  auto out = torch::empty({B, D + p_pad}, emb.options());
  int blocks = (B + 3) / 4;
  size_t lds = 4 * (size_t)F * D * sizeof(short);
  k_interact_cat_fwd<<<blocks, 256, lds, current_hip_stream()>>>(
      bf_ptr(bot), bf_ptr(emb), B, Fe, D, P, (int)p_pad, bf_ptr_mut(out));
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> interact_cat_bwd(
    torch::Tensor grad, torch::Tensor bot, torch::Tensor emb) {
  int B = emb.size(0), Fe = emb.size(1), D = emb.size(2);
  int F = Fe + 1;
  TORCH_CHECK(F <= 40, "interact: pair LUT supports F <= 40");
  int P = F * (F - 1) / 2;
  int P_pad = grad.size(1) - D;
  auto dbot = torch::empty_like(bot);
  auto demb = torch::empty_like(emb);
  int blocks = (B + 3) / 4;
  size_t lds = 4 * (size_t)(F * D + ((P + 7) & ~7)) * sizeof(short);
  k_interact_cat_bwd<<<blocks, 256, lds, current_hip_stream()>>>(
      bf_ptr(grad.contiguous()), bf_ptr(bot), bf_ptr(emb), B, Fe, D, P,
      P_pad, bf_ptr_mut(dbot), bf_ptr_mut(demb));
  return {dbot, demb};
}

std::tuple<torch::Tensor, torch::Tensor> l2norm_fwd(torch::Tensor x,
                                                    double eps) {
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous());
  int M = x.size(0), N = x.size(1);
  auto y = torch::empty_like(x);
  auto inv = torch::empty({M}, x.options().dtype(torch::kFloat32));
  k_l2norm_fwd<<<(M + 3) / 4, 256, 0, current_hip_stream()>>>(
      bf_ptr(x), M, N, (float)eps, bf_ptr_mut(y), inv.data_ptr<float>());
  return {y, inv};
}

torch::Tensor l2norm_bwd(torch::Tensor dy, torch::Tensor y,
                         torch::Tensor inv) {
  int M = y.size(0), N = y.size(1);
  auto dx = torch::empty_like(y);
  k_l2norm_bwd<<<(M + 3) / 4, 256, 0, current_hip_stream()>>>(
      bf_ptr(dy.contiguous()), bf_ptr(y), inv.data_ptr<float>(), M, N,
      bf_ptr_mut(dx));
  return dx;
}

void register_dense(py::module_& mod) {
  mod.def("l2norm_fwd", &l2norm_fwd);
  mod.def("l2norm_bwd", &l2norm_bwd);
  mod.def("interact_fwd", &interact_fwd);
  mod.def("interact_bwd", &interact_bwd);
  mod.def("interact_cat_fwd", &interact_cat_fwd);
  mod.def("interact_cat_bwd", &interact_cat_bwd);
  mod.def("linear_fwd", &linear_fwd, py::arg("x"), py::arg("w"),
          py::arg("bias"), py::arg("act"), py::arg("variant") = -1);
  mod.def("linear_dx", &linear_dx, py::arg("g"), py::arg("w"),
          py::arg("prev_out") = py::none(), py::arg("prev_act") = 0);
  mod.def("linear_dw", &linear_dw, py::arg("g"), py::arg("x"),
          py::arg("want_bias"), py::arg("variant") = -1);
  mod.def("linear_dw_out", &linear_dw_out, py::arg("g"), py::arg("x"),
          py::arg("ws"), py::arg("want_bias"), py::arg("variant") = -1,
          py::arg("zero") = true);
  mod.def("zero_f32", &zero_f32, py::arg("ws"));
  mod.def("pad_cast_bf16", &pad_cast_bf16, py::arg("x"), py::arg("k_pad"));
  mod.def("dense_adam", &dense_adam);
  mod.def("resln_fwd", &resln_fwd);
  mod.def("resln_bwd", &resln_bwd);
  mod.def("act_bwd", &act_bwd);
}
