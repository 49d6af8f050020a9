// ev_read_kernels.hip — the embedding read surface for gfx950: unique-row
// gather, padded sequence gather, pooled forward and group pooled forward,
// each ONE kernel body instantiated per row source.
//
// Row sources (small structs passed to the kernel by value; load<VEC>()
// yields VEC fp32 elements of one row starting at column d0):
//   F32Rows    the fp32 value slab [slots, dim] of HbmStorage
//   Q8Rows     the fp8-resident slab of QuantizedHbmStorage: OCP e4m3 bytes
//              [slots, dim] plus one fp32 scale per row (the layout
//              tools/quantize_embeddings.py writes),
//                value(s, d) = fl32(scale[s] * decode_e4m3(q[s, d]))
//              one fp32 multiply per element, rounded BEFORE any weighting
//              or summation (exactly ops/fp8.py dequantize_fp8_rows)
//   DirectRows fp32 rows pre-gathered per unique key (the sharded path:
//              rows arrive from peer shards over RCCL all-to-all). Indexed
//              by the unique index, never missing; reads no slots or keys.
//
// Shared by every kernel: read_unique() (the row of a unique key, or the
// missing-key value), pool_bag() (fp32 accumulation over a bag in j order,
// then the combiner coefficient) and store_chunk() (one rounding to the
// output dtype, one store).
//
// Thread mapping: a thread owns a VEC-element chunk of one output row and
// consecutive threads take consecutive chunks, so a wave reads and writes
// whole rows back to back. The host picks VEC per row source (kVec* below);
// VEC == 1 is the scalar path for any dim. All four kernels grid-stride
// (see the NOTE on n_blocks in hip_common.h).

#include "hip_common.h"

#include <type_traits>

namespace py = pybind11;

#define DEV_INLINE __device__ __forceinline__

namespace {

constexpr int kBlock = 256;

// Widest chunk per row source; the launch takes the widest of {8, 4, 1}
// that is within this, divides dim and fits a 16-byte store.
constexpr int kVecF32 = 1;     // thread = one element
constexpr int kVecF32Seq = 8;  // k_seq_gather_pad is bound by its 16-B stores
constexpr int kVecQ8 = 4;      // one 32-bit load of four e4m3 bytes
constexpr int kVecDirect = 1;

using f32x2 = __attribute__((ext_vector_type(2))) float;

// VEC fp32 elements at src (16-B aligned when VEC % 4 == 0: dim % 4 == 0).
template <int VEC>
DEV_INLINE void load_f32(const float* __restrict__ src, float (&v)[VEC]) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      const float4 q = *reinterpret_cast<const float4*>(src + i);
      v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
    }
  } else {
    static_assert(VEC == 1, "VEC is 8, 4 or 1");
    v[0] = src[0];
  }
}

struct F32Rows {
  const float* __restrict__ values;
  template <int VEC>
  DEV_INLINE void load(int64_t s, int dim, int d0, float (&v)[VEC]) const {
    load_f32<VEC>(values + s * dim + d0, v);
  }
};

struct Q8Rows {
  const uint8_t* __restrict__ values;
  const float* __restrict__ scales;
  template <int VEC>
  DEV_INLINE void load(int64_t s, int dim, int d0, float (&v)[VEC]) const {
    const float sc = scales[s];
    const uint8_t* src = values + s * dim + d0;
    if constexpr (VEC == 4) {
      // rows are 4-byte aligned: dim % 4 == 0 and d0 % 4 == 0
      const int word = (int)*reinterpret_cast<const uint32_t*>(src);
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(word, false);  // bytes 0,1
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(word, true);   // bytes 2,3
      v[0] = sc * lo.x; v[1] = sc * lo.y;
      v[2] = sc * hi.x; v[3] = sc * hi.y;
    } else {
      static_assert(VEC == 1, "VEC is 4 or 1");
      v[0] = sc * __builtin_amdgcn_cvt_f32_fp8((int)src[0], 0);
    }
  }
};

struct DirectRows {
  const float* __restrict__ rows;
  template <int VEC>
  DEV_INLINE void load(int64_t u, int dim, int d0, float (&v)[VEC]) const {
    load_f32<VEC>(rows + u * dim + d0, v);
  }
};

// What a slot-indexed source needs to serve a unique key: its slot, and the
// value a key without a slot reads. Unused (all zero) with DirectRows.
struct Missing {
  const float* __restrict__ default_values;
  const int64_t* __restrict__ keys;
  const int32_t* __restrict__ slots;
  int default_value_dim;  // default rows per table
  int64_t key_mask;       // the raw id inside a key; all ones for plain keys
  float no_permission_value;
  int use_no_permission;
};

// Row of default_values a missing key reads: the raw id hashed into its
// table's block of rows. Single-table kernels pass table 0 and a key_mask
// of all ones (kWholeKey), which makes it key % default_value_dim.
DEV_INLINE int64_t missing_default_row(int64_t key, int table,
                                       int64_t key_mask,
                                       int default_value_dim) {
  return (int64_t)table * default_value_dim +
         (int64_t)((uint64_t)(key & key_mask) % (uint64_t)default_value_dim);
}

// One chunk of unique key u: slot >= 0 -> the stored row; else the
// no-permission value; else the key's default_values row.
template <typename Rows, int VEC>
DEV_INLINE void read_unique(const Rows& rows, const Missing& miss, int u,
                            int table, int dim, int d0, float (&v)[VEC]) {
  if constexpr (std::is_same_v<Rows, DirectRows>) {
    rows.template load<VEC>(u, dim, d0, v);
  } else {
    const int32_t s = miss.slots[u];
    if (s >= 0) {
      rows.template load<VEC>(s, dim, d0, v);
    } else if (miss.use_no_permission) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = miss.no_permission_value;
    } else {
      const int64_t row = missing_default_row(
          miss.keys[u], table, miss.key_mask, miss.default_value_dim);
      load_f32<VEC>(miss.default_values + row * dim + d0, v);
    }
  }
}

// One rounding to OutT and one store of the chunk; bf16 pairs are packed
// into 32-bit words (dst is VEC * sizeof(OutT)-byte aligned).
template <typename OutT, int VEC>
DEV_INLINE void store_chunk(OutT* __restrict__ dst, const float (&v)[VEC]) {
  if constexpr (std::is_same_v<OutT, __hip_bfloat16>) {
    if constexpr (VEC == 1) {
      dst[0] = __float2bfloat16(v[0]);
    } else {
      uint32_t w[VEC / 2];
#pragma unroll
      for (int i = 0; i < VEC / 2; ++i) {
        const __hip_bfloat16 lo = __float2bfloat16(v[2 * i]);
        const __hip_bfloat16 hi = __float2bfloat16(v[2 * i + 1]);
        w[i] = (uint32_t)(*reinterpret_cast<const uint16_t*>(&lo)) |
               ((uint32_t)(*reinterpret_cast<const uint16_t*>(&hi)) << 16);
      }
      if constexpr (VEC == 8)
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
      else
        *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
    }
  } else {
    static_assert(VEC == 4 || VEC == 1, "fp32 chunks are 4 or 1 wide");
    if constexpr (VEC == 4)
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else
      dst[0] = v[0];
  }
}

// acc = coeff * sum_j w_j * row(inverse[j]) over the bag [beg, end), summed
// in fp32 in j order. combiner: 0 = sum, 1 = mean (coeff 1 / sum w),
// 2 = sqrtn (coeff 1 / sqrt(sum w^2)); weights == nullptr means w = 1.
template <typename Rows, int VEC>
DEV_INLINE void pool_bag(const Rows& rows, const Missing& miss,
                         const int32_t* __restrict__ inverse,
                         const float* __restrict__ weights, int beg, int end,
                         int table, int combiner, int dim, int d0,
                         float (&acc)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
  float wacc = 0.0f;
  for (int j = beg; j < end; ++j) {
    float v[VEC];
    read_unique<Rows, VEC>(rows, miss, inverse[j], table, dim, d0, v);
    const float w = weights ? weights[j] : 1.0f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] += w * v[i];
    wacc += (combiner == 2) ? w * w : w;
  }
  float coeff = 1.0f;
  if (combiner != 0 && end > beg) {
    const float denom = (combiner == 2) ? sqrtf(wacc) : wacc;
    coeff = denom > 1e-12f ? 1.0f / denom : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] *= coeff;
}

// Plain gather of unique rows: out[i] = row of unique key i.
template <typename Rows, typename OutT, int VEC>
__global__ void k_gather(Rows rows, Missing miss, int m, int dim,
                         OutT* __restrict__ out) {
  const int cpr = dim / VEC;  // chunks per row
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)m * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int i = (int)(t / cpr);
    const int d0 = (int)(t % cpr) * VEC;
    float v[VEC];
    read_unique<Rows, VEC>(rows, miss, i, 0, dim, d0, v);
    store_chunk<OutT, VEC>(out + (int64_t)i * dim + d0, v);
  }
}

// Unpooled gather over a padded stream (sequence features):
//   out[j, :] = 0                          where inverse[j] < 0 (padding)
//   out[j, :] = row of unique key inverse[j] otherwise.
// slots/keys may be nnz-padded (capture): only rows a valid inverse names
// are read, and an inverse past n_uniq is treated as padding, never
// dereferenced. Memory-bound on the [nnz, dim] write.
template <typename Rows, typename OutT, int VEC>
__global__ void k_seq_gather_pad(Rows rows, Missing miss,
                                 const int32_t* __restrict__ inverse, int nnz,
                                 int n_uniq, int dim, OutT* __restrict__ out) {
  const int cpr = dim / VEC;
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)nnz * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int j = (int)(t / cpr);
    const int d0 = (int)(t % cpr) * VEC;
    const int u = inverse[j];
    float v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = 0.0f;
    if ((unsigned)u < (unsigned)n_uniq)
      read_unique<Rows, VEC>(rows, miss, u, 0, dim, d0, v);
    store_chunk<OutT, VEC>(out + (int64_t)j * dim + d0, v);
  }
}

// Fused gather + segment pooling. Thread = (batch row b, chunk of dim); no
// [nnz, dim] or [m, dim] intermediate is materialized.
template <typename Rows, typename OutT, int VEC>
__global__ void k_pooled_fwd(Rows rows, Missing miss,
                             const int32_t* __restrict__ inverse,
                             const int32_t* __restrict__ offsets,
                             const float* __restrict__ weights, int batch,
                             int dim, int combiner, OutT* __restrict__ out) {
  const int cpr = dim / VEC;
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)batch * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int b = (int)(t / cpr);
    const int d0 = (int)(t % cpr) * VEC;
    float acc[VEC];
    pool_bag<Rows, VEC>(rows, miss, inverse, weights, offsets[b],
                        offsets[b + 1], 0, combiner, dim, d0, acc);
    store_chunk<OutT, VEC>(out + (int64_t)b * dim + d0, acc);
  }
}

// Grouped (multi-table) fused pooling — the EmbeddingCollection hot path.
// N tables of equal dim share one storage via composite keys
// (table_id << key_bits) | id: one unique + one probe + ONE launch per step
// regardless of table count. The N tables' ragged batches are concatenated:
// offsets[(N*B)+1]; pooled row rid (< N*B) is table rid / B, sample rid % B.
// Output is interleaved as out[b, table*D + d], the [B, N*D] concat layout
// models consume with no extra copy.
template <typename Rows, typename OutT, int VEC>
__global__ void k_group_pooled_fwd(
    Rows rows, Missing miss, const int32_t* __restrict__ inverse,
    const int32_t* __restrict__ offsets, const float* __restrict__ weights,
    const int32_t* __restrict__ combiner_ids, int batch, int n_tables,
    int dim, OutT* __restrict__ out) {
  const int cpr = dim / VEC;
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)batch * n_tables * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int d0 = (int)(t % cpr) * VEC;
    const int64_t rid = t / cpr;  // pooled row in [0, N*B)
    const int table = (int)(rid / batch);
    const int b = (int)(rid % batch);
    float acc[VEC];
    pool_bag<Rows, VEC>(rows, miss, inverse, weights, offsets[rid],
                        offsets[rid + 1], table, combiner_ids[table], dim, d0,
                        acc);
    store_chunk<OutT, VEC>(
        out + ((int64_t)b * n_tables + table) * dim + d0, acc);
  }
}

}  // namespace

// ------------------------------------------------------------------
// host side
// ------------------------------------------------------------------

// Calls f(OutT*, integral_constant<int, VEC>) for the output dtype and the
// widest VEC of {8, 4, 1} that is <= MAXVEC, divides dim and stores at most
// 16 bytes. Only the reachable (OutT, VEC) pairs are instantiated.
template <int MAXVEC, typename OutT, typename F>
static void dispatch_vec(OutT* op, int dim, F&& f) {
  if constexpr (MAXVEC >= 8 && sizeof(OutT) * 8 <= 16) {
    if (dim % 8 == 0) return f(op, std::integral_constant<int, 8>{});
  }
  if constexpr (MAXVEC >= 4) {
    if (dim % 4 == 0) return f(op, std::integral_constant<int, 4>{});
  }
  f(op, std::integral_constant<int, 1>{});
}

template <int MAXVEC, typename F>
static void dispatch_out_vec(torch::Tensor& out, int dim, F&& f) {
  if (out.scalar_type() == torch::kBFloat16)
    dispatch_vec<MAXVEC>(
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr<at::BFloat16>()), dim,
        f);
  else
    dispatch_vec<MAXVEC>(out.data_ptr<float>(), dim, f);
}

constexpr int64_t kWholeKey = -1;  // key_mask of plain (single-table) keys

static Missing missing_keys(const torch::Tensor& default_values,
                            const torch::Tensor& keys,
                            const torch::Tensor& slots, int64_t n_tables,
                            int64_t key_mask, double no_permission_value,
                            bool use_no_permission) {
  return {default_values.data_ptr<float>(), keys.data_ptr<int64_t>(),
          slots.data_ptr<int32_t>(),
          (int)(default_values.size(0) / n_tables), key_mask,
          (float)no_permission_value, use_no_permission ? 1 : 0};
}

static const float* weights_or_null(const torch::Tensor& weights) {
  return weights.defined() && weights.numel() ? weights.data_ptr<float>()
                                              : nullptr;
}

template <int MAXVEC, typename Rows>
static void launch_gather(Rows rows, const Missing& miss, int m, int dim,
                          torch::Tensor& out) {
  auto stream = current_hip_stream();
  dispatch_out_vec<MAXVEC>(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_gather<Rows, OutT, VEC>
        <<<n_blocks((int64_t)m * (dim / VEC)), kBlock, 0, stream>>>(
            rows, miss, m, dim, op);
  });
}

template <int MAXVEC, typename Rows>
static void launch_seq_gather_pad(Rows rows, const Missing& miss,
                                  const torch::Tensor& inverse, int n_uniq,
                                  int dim, torch::Tensor& out) {
  auto stream = current_hip_stream();
  const int64_t nnz = inverse.numel();
  dispatch_out_vec<MAXVEC>(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_seq_gather_pad<Rows, OutT, VEC>
        <<<n_blocks(nnz * (dim / VEC)), kBlock, 0, stream>>>(
            rows, miss, inverse.data_ptr<int32_t>(), (int)nnz, n_uniq, dim,
            op);
  });
}

template <int MAXVEC, typename Rows>
static void launch_pooled_fwd(Rows rows, const Missing& miss,
                              const torch::Tensor& inverse,
                              const torch::Tensor& offsets,
                              const torch::Tensor& weights, int batch,
                              int dim, int64_t combiner, torch::Tensor& out) {
  auto stream = current_hip_stream();
  const float* wptr = weights_or_null(weights);
  dispatch_out_vec<MAXVEC>(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_pooled_fwd<Rows, OutT, VEC>
        <<<n_blocks((int64_t)batch * (dim / VEC)), kBlock, 0, stream>>>(
            rows, miss, inverse.data_ptr<int32_t>(),
            offsets.data_ptr<int32_t>(), wptr, batch, dim, (int)combiner, op);
  });
}

template <int MAXVEC, typename Rows>
static void launch_group_pooled_fwd(
    Rows rows, const Missing& miss, const torch::Tensor& inverse,
    const torch::Tensor& offsets, const torch::Tensor& weights,
    const torch::Tensor& combiner_ids, int64_t batch, int64_t n_tables,
    int dim, torch::Tensor& out) {
  auto stream = current_hip_stream();
  const float* wptr = weights_or_null(weights);
  dispatch_out_vec<MAXVEC>(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_group_pooled_fwd<Rows, OutT, VEC>
        <<<n_blocks(batch * n_tables * (dim / VEC)), kBlock, 0, stream>>>(
            rows, miss, inverse.data_ptr<int32_t>(),
            offsets.data_ptr<int32_t>(), wptr,
            combiner_ids.data_ptr<int32_t>(), (int)batch, (int)n_tables, dim,
            op);
  });
}

// --- fp32 rows -------------------------------------------------------

torch::Tensor ev_gather(torch::Tensor values, torch::Tensor default_values,
                        torch::Tensor keys, torch::Tensor slots,
                        double no_permission_value, bool use_no_permission,
                        torch::ScalarType out_dtype) {
  int m = keys.numel();
  int dim = values.size(1);
  auto out = torch::empty({m, dim}, values.options().dtype(out_dtype));
  if (m == 0) return out;
  launch_gather<kVecF32>(
      F32Rows{values.data_ptr<float>()},
      missing_keys(default_values, keys, slots, 1, kWholeKey,
                   no_permission_value, use_no_permission),
      m, dim, out);
  return out;
}

// out [nnz, dim]: zero rows where inverse < 0, else the row of
// slots[inverse] (see k_seq_gather_pad). keys/slots may be nnz-padded.
torch::Tensor seq_gather_pad(torch::Tensor values,
                             torch::Tensor default_values, torch::Tensor keys,
                             torch::Tensor slots, torch::Tensor inverse,
                             double no_permission_value,
                             bool use_no_permission,
                             torch::ScalarType out_dtype) {
  TORCH_CHECK(inverse.is_cuda(), "inverse must be on GPU");
  TORCH_CHECK(keys.numel() == slots.numel(),
              "seq_gather_pad: keys/slots size mismatch");
  TORCH_CHECK(out_dtype == torch::kFloat32 || out_dtype == torch::kBFloat16,
              "seq_gather_pad: out dtype must be float32 or bfloat16");
  int64_t nnz = inverse.numel();
  int dim = values.size(1);
  auto out = torch::empty({nnz, dim}, values.options().dtype(out_dtype));
  if (nnz * dim == 0) return out;
  launch_seq_gather_pad<kVecF32Seq>(
      F32Rows{values.data_ptr<float>()},
      missing_keys(default_values, keys, slots, 1, kWholeKey,
                   no_permission_value, use_no_permission),
      inverse, (int)slots.numel(), dim, out);
  return out;
}

torch::Tensor pooled_fwd(torch::Tensor values, torch::Tensor default_values,
                         torch::Tensor keys, torch::Tensor slots,
                         torch::Tensor inverse, torch::Tensor offsets,
                         torch::Tensor weights, int64_t combiner,
                         double no_permission_value, bool use_no_permission,
                         torch::ScalarType out_dtype) {
  int batch = offsets.numel() - 1;
  int dim = values.size(1);
  auto out = torch::empty({batch, dim}, values.options().dtype(out_dtype));
  if (batch == 0) return out;
  launch_pooled_fwd<kVecF32>(
      F32Rows{values.data_ptr<float>()},
      missing_keys(default_values, keys, slots, 1, kWholeKey,
                   no_permission_value, use_no_permission),
      inverse, offsets, weights, batch, dim, combiner, out);
  return out;
}

torch::Tensor group_pooled_fwd(
    torch::Tensor values, torch::Tensor default_values, torch::Tensor keys,
    torch::Tensor slots, torch::Tensor inverse, torch::Tensor offsets,
    torch::Tensor weights, torch::Tensor combiner_ids, int64_t batch,
    int64_t n_tables, int64_t key_bits, double no_permission_value,
    bool use_no_permission, torch::ScalarType out_dtype) {
  int dim = values.size(1);
  auto out = torch::empty({batch, n_tables * dim},
                          values.options().dtype(out_dtype));
  if (batch * n_tables * dim == 0) return out;
  launch_group_pooled_fwd<kVecF32>(
      F32Rows{values.data_ptr<float>()},
      missing_keys(default_values, keys, slots, n_tables,
                   ((int64_t)1 << key_bits) - 1, no_permission_value,
                   use_no_permission),
      inverse, offsets, weights, combiner_ids, batch, n_tables, dim, out);
  return out;
}

// --- pre-gathered rows (sharded path) --------------------------------

torch::Tensor group_pooled_fwd_direct(
    torch::Tensor emb_rows, torch::Tensor keys, torch::Tensor inverse,
    torch::Tensor offsets, torch::Tensor weights, torch::Tensor combiner_ids,
    int64_t batch, int64_t n_tables, torch::ScalarType out_dtype) {
  int dim = emb_rows.size(1);
  auto out = torch::empty({batch, n_tables * dim},
                          emb_rows.options().dtype(out_dtype));
  if (batch * n_tables * dim == 0) return out;
  // the rows are already per unique key: `keys` is only type-checked
  TORCH_CHECK(keys.scalar_type() == torch::kInt64,
              "group_pooled_fwd_direct: keys must be int64");
  launch_group_pooled_fwd<kVecDirect>(
      DirectRows{emb_rows.data_ptr<float>()}, Missing{}, inverse, offsets,
      weights, combiner_ids, batch, n_tables, dim, out);
  return out;
}

// --- fp8-resident rows -----------------------------------------------

static void check_q8(const torch::Tensor& values, const torch::Tensor& scales,
                     const torch::Tensor& default_values,
                     torch::ScalarType out_dtype) {
  TORCH_CHECK(values.is_cuda() && values.dim() == 2 &&
                  values.is_contiguous() &&
                  values.scalar_type() == torch::kUInt8,
              "q8: values must be a contiguous uint8 [slots, dim] on GPU");
  TORCH_CHECK(scales.is_cuda() && scales.is_contiguous() &&
                  scales.scalar_type() == torch::kFloat32 &&
                  scales.numel() == values.size(0),
              "q8: scales must be fp32 [slots] on GPU");
  TORCH_CHECK(default_values.scalar_type() == torch::kFloat32 &&
                  default_values.is_contiguous() &&
                  default_values.size(1) == values.size(1),
              "q8: default_values must be fp32 [rows, dim]");
  TORCH_CHECK(out_dtype == torch::kFloat32 || out_dtype == torch::kBFloat16,
              "q8: out dtype must be float32 or bfloat16");
}

torch::Tensor ev_gather_q8(torch::Tensor values, torch::Tensor scales,
                           torch::Tensor default_values, torch::Tensor keys,
                           torch::Tensor slots, double no_permission_value,
                           bool use_no_permission,
                           torch::ScalarType out_dtype) {
  check_q8(values, scales, default_values, out_dtype);
  TORCH_CHECK(keys.numel() == slots.numel(),
              "ev_gather_q8: keys/slots size mismatch");
  const int m = (int)keys.numel();
  const int dim = (int)values.size(1);
  auto out = torch::empty({m, dim}, values.options().dtype(out_dtype));
  if ((int64_t)m * dim == 0) return out;
  launch_gather<kVecQ8>(
      Q8Rows{values.data_ptr<uint8_t>(), scales.data_ptr<float>()},
      missing_keys(default_values, keys, slots, 1, kWholeKey,
                   no_permission_value, use_no_permission),
      m, dim, out);
  return out;
}

torch::Tensor seq_gather_pad_q8(torch::Tensor values, torch::Tensor scales,
                                torch::Tensor default_values,
                                torch::Tensor keys, torch::Tensor slots,
                                torch::Tensor inverse,
                                double no_permission_value,
                                bool use_no_permission,
                                torch::ScalarType out_dtype) {
  check_q8(values, scales, default_values, out_dtype);
  TORCH_CHECK(inverse.is_cuda(), "inverse must be on GPU");
  TORCH_CHECK(keys.numel() == slots.numel(),
              "seq_gather_pad_q8: keys/slots size mismatch");
  const int64_t nnz = inverse.numel();
  const int dim = (int)values.size(1);
  auto out = torch::empty({nnz, dim}, values.options().dtype(out_dtype));
  if (nnz * dim == 0) return out;
  launch_seq_gather_pad<kVecQ8>(
      Q8Rows{values.data_ptr<uint8_t>(), scales.data_ptr<float>()},
      missing_keys(default_values, keys, slots, 1, kWholeKey,
                   no_permission_value, use_no_permission),
      inverse, (int)slots.numel(), dim, out);
  return out;
}

torch::Tensor pooled_fwd_q8(torch::Tensor values, torch::Tensor scales,
                            torch::Tensor default_values, torch::Tensor keys,
                            torch::Tensor slots, torch::Tensor inverse,
                            torch::Tensor offsets, torch::Tensor weights,
                            int64_t combiner, double no_permission_value,
                            bool use_no_permission,
                            torch::ScalarType out_dtype) {
  check_q8(values, scales, default_values, out_dtype);
  const int batch = (int)offsets.numel() - 1;
  const int dim = (int)values.size(1);
  auto out = torch::empty({batch, dim}, values.options().dtype(out_dtype));
  if ((int64_t)batch * dim == 0) return out;
  launch_pooled_fwd<kVecQ8>(
      Q8Rows{values.data_ptr<uint8_t>(), scales.data_ptr<float>()},
      missing_keys(default_values, keys, slots, 1, kWholeKey,
                   no_permission_value, use_no_permission),
      inverse, offsets, weights, batch, dim, combiner, out);
  return out;
}

torch::Tensor group_pooled_fwd_q8(
    torch::Tensor values, torch::Tensor scales, torch::Tensor default_values,
    torch::Tensor keys, torch::Tensor slots, torch::Tensor inverse,
    torch::Tensor offsets, torch::Tensor weights, torch::Tensor combiner_ids,
    int64_t batch, int64_t n_tables, int64_t key_bits,
    double no_permission_value, bool use_no_permission,
    torch::ScalarType out_dtype) {
  check_q8(values, scales, default_values, out_dtype);
  const int dim = (int)values.size(1);
  auto out = torch::empty({batch, n_tables * dim},
                          values.options().dtype(out_dtype));
  if (batch * n_tables * dim == 0) return out;
  TORCH_CHECK(offsets.numel() == batch * n_tables + 1,
              "group_pooled_fwd_q8: offsets must hold N*B+1 entries");
  launch_group_pooled_fwd<kVecQ8>(
      Q8Rows{values.data_ptr<uint8_t>(), scales.data_ptr<float>()},
      missing_keys(default_values, keys, slots, n_tables,
                   ((int64_t)1 << key_bits) - 1, no_permission_value,
                   use_no_permission),
      inverse, offsets, weights, combiner_ids, batch, n_tables, dim, out);
  return out;
}

void register_ev_read(py::module_& mod) {
  mod.def("ev_gather", &ev_gather);
  mod.def("seq_gather_pad", &seq_gather_pad);
  mod.def("pooled_fwd", &pooled_fwd);
  mod.def("group_pooled_fwd", &group_pooled_fwd);
  mod.def("group_pooled_fwd_direct", &group_pooled_fwd_direct);
  mod.def("ev_gather_q8", &ev_gather_q8);
  mod.def("seq_gather_pad_q8", &seq_gather_pad_q8);
  mod.def("pooled_fwd_q8", &pooled_fwd_q8);
  mod.def("group_pooled_fwd_q8", &group_pooled_fwd_q8);
}
