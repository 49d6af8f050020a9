// swz_tile.h — the swizzled bf16 LDS tile of the per-position MLP kernels
// (din_attention_kernels.hip, dien_aux_kernels.hip) and the small helpers
// both use around it.
//
// LDS tiles. [rows][64] bf16 per 64 columns, 128-B rows, no padding, read
// two ways: 16-B row fragments (16 lanes: 16 rows x one 16-B piece) and
// transposed 8-B reads (32 lanes: 8 rows x one 32-B block). Bank = dword
// % 64; the row's bit 0 picks the half of the banks; the 32-B block index
// is XORed with bits 1-2 of the row and the 16-B half inside the block with
// bit 3, so the 8 rows of equal parity in a row-fragment read hit 8
// different 16-B slots, and the 8 rows of a transposed read (bit 3 fixed)
// 8 different 32-B blocks: both conflict-free.
// Rules of the transposed read: EXEC all ones (wave-uniform branches only)
// and every lane's address inside the tile.
#pragma once

#include "mfma_fwd.h"

namespace {

using bf16x4 = __attribute__((ext_vector_type(4))) short;
typedef f32x4 f32x4_u __attribute__((aligned(4)));

// element offset of tile[row][col..] in a [rows][64 per column tile] LDS
// tile; col % 4 == 0 for 8-B and col % 8 == 0 for 16-B accesses
__device__ __forceinline__ int da_off(int rows, int row, int col) {
  return (col >> 6) * (rows * 64) + row * 64 +
         (((((col >> 4) & 3) ^ ((row >> 1) & 3)) << 4) |
          ((col & 15) ^ (((row >> 3) & 1) << 3)));
}

__host__ __device__ inline int da_tile_elems(int rows, int cols) {
  return rows * 64 * ((cols + 63) / 64);
}

// Transposed fragment of tile rows r0 + 4 (lane / 16) + q, columns
// c0 .. c0 + 15: lane 4 q + p of a 16-lane group supplies row q, columns
// c0 + 4 p ..; lane i of the group receives column c0 + i, row q in
// element q — the A (row = column index) or B operand of a 16x16x16 MFMA
// whose k runs over the tile's rows.
__device__ __forceinline__ bf16x4 da_read_tr(const short* tile, int rows,
                                             int r0, int c0, int lane) {
  const int row = r0 + 4 * (lane >> 4) + ((lane >> 2) & 3);
  const short* p = tile + da_off(rows, row, c0 + 4 * (lane & 3));
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

__device__ __forceinline__ f32x4 mfma16(bf16x4 a, bf16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float da_sigmoid(float v) {
  return 1.0f / (1.0f + __expf(-v));
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// sum over the 16 lanes of equal lane / 16
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

}  // namespace
