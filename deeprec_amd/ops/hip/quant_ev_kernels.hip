// quant_ev_kernels.hip — read path of the fp8-resident embedding storage
// (ops/quant_backend.py, QuantizedHbmStorage) for gfx950.
//
// The value slab is OCP e4m3 bytes [slots, dim] with one fp32 scale per row
// in a separate [slots] array (the layout tools/quantize_embeddings.py
// writes), 20 B per dim-16 row instead of 64 B. The four kernels mirror the
// fp32 read surface of ev_kernels.hip (k_gather, k_seq_gather_pad,
// k_pooled_fwd, k_group_pooled_fwd) and dequantize inside the gather:
//
//   value(s, d) = fl32(scale[s] * decode_e4m3(q[s, d]))
//
// one fp32 multiply per element, rounded BEFORE any weighting or summation
// (exactly ops/fp8.py dequantize_fp8_rows), then the fp32 kernels'
// arithmetic unchanged: fp32 accumulation over the bag in j order, the
// combiner coefficient, one rounding to the output dtype. Missing keys
// (slot < 0) read the fp32 default_values row or the no-permission value as
// the fp32 kernels do.
//
// Thread mapping: a thread owns a VEC-element chunk of one output row, not
// one element — byte-wide elements under the fp32 kernels' mapping would be
// 1-byte loads. VEC = 4 when dim % 4 == 0: one 32-bit load per row visit,
// decoded by two v_cvt_pk_f32_fp8 (low and high half of the word); VEC = 1
// is the scalar byte path for any other dim. All four grid-stride (see the
// NOTE on n_blocks in hip_common.h).

#include "hip_common.h"

#include <type_traits>

namespace py = pybind11;

namespace {

constexpr int kBlock = 256;

using f32x2 = __attribute__((ext_vector_type(2))) float;

// VEC dequantized elements of row s starting at column d0.
template <int VEC>
__device__ __forceinline__ void load_row_q8(
    const uint8_t* __restrict__ values, const float* __restrict__ scales,
    int32_t s, int dim, int d0, float (&v)[VEC]) {
  const float sc = scales[s];
  const uint8_t* src = values + (int64_t)s * dim + d0;
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

// VEC fp32 elements of a default_values row (16-B aligned when VEC == 4).
template <int VEC>
__device__ __forceinline__ void load_row_f32(const float* __restrict__ src,
                                             float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(src);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = src[0];
  }
}

// One chunk of unique row u: the quantized row when it has a slot, else the
// fp32 kernels' missing-key value. `drow` is the default_values row.
template <int VEC>
__device__ __forceinline__ void load_chunk(
    const uint8_t* __restrict__ values, const float* __restrict__ scales,
    const float* __restrict__ default_values, int32_t s, int64_t drow,
    int dim, int d0, float no_permission_value, int use_no_permission,
    float (&v)[VEC]) {
  if (s >= 0) {
    load_row_q8<VEC>(values, scales, s, dim, d0, v);
  } else if (use_no_permission) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = no_permission_value;
  } else {
    load_row_f32<VEC>(default_values + drow * dim + d0, v);
  }
}

// One rounding to OutT and one store of the chunk; bf16 pairs are packed
// into 32-bit words as k_seq_gather_pad does (dst is 8-B aligned at VEC 4).
template <typename OutT, int VEC>
__device__ __forceinline__ void store_chunk(OutT* __restrict__ dst,
                                            const float (&v)[VEC]) {
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
      *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
    }
  } else {
    if constexpr (VEC == 4)
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else
      dst[0] = v[0];
  }
}

// out[i] = dequantized row of slots[i], or the missing-key value.
template <typename OutT, int VEC>
__global__ void k_gather_q8(
    const uint8_t* __restrict__ values, const float* __restrict__ scales,
    const float* __restrict__ default_values,
    const int64_t* __restrict__ keys, const int32_t* __restrict__ slots,
    int m, int dim, int default_value_dim, float no_permission_value,
    int use_no_permission, OutT* __restrict__ out) {
  const int cpr = dim / VEC;  // chunks per row
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)m * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int i = (int)(t / cpr);
    const int d0 = (int)(t % cpr) * VEC;
    const int32_t s = slots[i];
    int64_t drow = 0;
    if (s < 0 && !use_no_permission)
      drow = (int64_t)((uint64_t)keys[i] % (uint64_t)default_value_dim);
    float v[VEC];
    load_chunk<VEC>(values, scales, default_values, s, drow, dim, d0,
                    no_permission_value, use_no_permission, v);
    store_chunk<OutT, VEC>(out + (int64_t)i * dim + d0, v);
  }
}

// k_seq_gather_pad over quantized rows: zero rows where inverse[j] < 0 or
// inverse[j] >= n_uniq (never dereferenced); keys/slots may be nnz-padded.
template <typename OutT, int VEC>
__global__ void k_seq_gather_pad_q8(
    const uint8_t* __restrict__ values, const float* __restrict__ scales,
    const float* __restrict__ default_values,
    const int64_t* __restrict__ keys, const int32_t* __restrict__ slots,
    const int32_t* __restrict__ inverse, int nnz, int n_uniq, int dim,
    int default_value_dim, float no_permission_value, int use_no_permission,
    OutT* __restrict__ out) {
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
    if ((unsigned)u < (unsigned)n_uniq) {
      const int32_t s = slots[u];
      int64_t drow = 0;
      if (s < 0 && !use_no_permission)
        drow = (int64_t)((uint64_t)keys[u] % (uint64_t)default_value_dim);
      load_chunk<VEC>(values, scales, default_values, s, drow, dim, d0,
                      no_permission_value, use_no_permission, v);
    }
    store_chunk<OutT, VEC>(out + (int64_t)j * dim + d0, v);
  }
}

// k_pooled_fwd over quantized rows. Thread = (batch row b, chunk of dim).
template <typename OutT, int VEC>
__global__ void k_pooled_fwd_q8(
    const uint8_t* __restrict__ values, const float* __restrict__ scales,
    const float* __restrict__ default_values,
    const int64_t* __restrict__ keys, const int32_t* __restrict__ slots,
    const int32_t* __restrict__ inverse, const int32_t* __restrict__ offsets,
    const float* __restrict__ weights, int batch, int dim,
    int default_value_dim, float no_permission_value, int use_no_permission,
    int combiner, OutT* __restrict__ out) {
  const int cpr = dim / VEC;
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)batch * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    const int b = (int)(t / cpr);
    const int d0 = (int)(t % cpr) * VEC;
    const int beg = offsets[b], end = offsets[b + 1];
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
    float wacc = 0.0f;
    for (int j = beg; j < end; ++j) {
      const int u = inverse[j];
      const int32_t s = slots[u];
      int64_t drow = 0;
      if (s < 0 && !use_no_permission)
        drow = (int64_t)((uint64_t)keys[u] % (uint64_t)default_value_dim);
      float v[VEC];
      load_chunk<VEC>(values, scales, default_values, s, drow, dim, d0,
                      no_permission_value, use_no_permission, v);
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
    store_chunk<OutT, VEC>(out + (int64_t)b * dim + d0, acc);
  }
}

// k_group_pooled_fwd over quantized rows (no `direct` variant): pooled row
// rid (< N*B) is table rid / B, sample rid % B; output interleaved as
// out[b, table*D + d].
template <typename OutT, int VEC>
__global__ void k_group_pooled_fwd_q8(
    const uint8_t* __restrict__ values, const float* __restrict__ scales,
    const float* __restrict__ default_values,
    const int64_t* __restrict__ keys, const int32_t* __restrict__ slots,
    const int32_t* __restrict__ inverse, const int32_t* __restrict__ offsets,
    const float* __restrict__ weights,
    const int32_t* __restrict__ combiner_ids, int batch, int n_tables,
    int dim, int default_value_dim, int key_bits, float no_permission_value,
    int use_no_permission, OutT* __restrict__ out) {
  const int cpr = dim / VEC;
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)batch * n_tables * cpr;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t key_mask = ((int64_t)1 << key_bits) - 1;
  for (; t < total; t += stride) {
    const int d0 = (int)(t % cpr) * VEC;
    const int64_t rid = t / cpr;  // pooled row in [0, N*B)
    const int table = (int)(rid / batch);
    const int b = (int)(rid % batch);
    const int beg = offsets[rid], end = offsets[rid + 1];
    const int combiner = combiner_ids[table];
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
    float wacc = 0.0f;
    for (int j = beg; j < end; ++j) {
      const int u = inverse[j];
      const int32_t s = slots[u];
      int64_t drow = 0;
      if (s < 0 && !use_no_permission)
        drow = (int64_t)table * default_value_dim +
               (int64_t)((uint64_t)(keys[u] & key_mask) %
                         (uint64_t)default_value_dim);
      float v[VEC];
      load_chunk<VEC>(values, scales, default_values, s, drow, dim, d0,
                      no_permission_value, use_no_permission, v);
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
    store_chunk<OutT, VEC>(
        out + ((int64_t)b * n_tables + table) * dim + d0, acc);
  }
}

}  // namespace

// ------------------------------------------------------------------
// wrappers
// ------------------------------------------------------------------

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

// Calls f(OutT*, integral_constant<int, VEC>) for the output dtype and the
// widest VEC the row width allows.
template <typename F>
static void dispatch_out_vec(torch::Tensor& out, int dim, F&& f) {
  using V4 = std::integral_constant<int, 4>;
  using V1 = std::integral_constant<int, 1>;
  if (out.scalar_type() == torch::kBFloat16) {
    auto* op = reinterpret_cast<__hip_bfloat16*>(out.data_ptr<at::BFloat16>());
    if (dim % 4 == 0) f(op, V4{});
    else f(op, V1{});
  } else {
    auto* op = out.data_ptr<float>();
    if (dim % 4 == 0) f(op, V4{});
    else f(op, V1{});
  }
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
  auto stream = current_hip_stream();
  dispatch_out_vec(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_gather_q8<OutT, VEC>
        <<<n_blocks((int64_t)m * (dim / VEC)), kBlock, 0, stream>>>(
            values.data_ptr<uint8_t>(), scales.data_ptr<float>(),
            default_values.data_ptr<float>(), keys.data_ptr<int64_t>(),
            slots.data_ptr<int32_t>(), m, dim, (int)default_values.size(0),
            (float)no_permission_value, use_no_permission ? 1 : 0, op);
  });
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
  auto stream = current_hip_stream();
  dispatch_out_vec(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_seq_gather_pad_q8<OutT, VEC>
        <<<n_blocks(nnz * (dim / VEC)), kBlock, 0, stream>>>(
            values.data_ptr<uint8_t>(), scales.data_ptr<float>(),
            default_values.data_ptr<float>(), keys.data_ptr<int64_t>(),
            slots.data_ptr<int32_t>(), inverse.data_ptr<int32_t>(), (int)nnz,
            (int)slots.numel(), dim, (int)default_values.size(0),
            (float)no_permission_value, use_no_permission ? 1 : 0, op);
  });
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
  auto stream = current_hip_stream();
  const float* wptr =
      weights.defined() && weights.numel() ? weights.data_ptr<float>()
                                           : nullptr;
  dispatch_out_vec(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_pooled_fwd_q8<OutT, VEC>
        <<<n_blocks((int64_t)batch * (dim / VEC)), kBlock, 0, stream>>>(
            values.data_ptr<uint8_t>(), scales.data_ptr<float>(),
            default_values.data_ptr<float>(), keys.data_ptr<int64_t>(),
            slots.data_ptr<int32_t>(), inverse.data_ptr<int32_t>(),
            offsets.data_ptr<int32_t>(), wptr, batch, dim,
            (int)default_values.size(0), (float)no_permission_value,
            use_no_permission ? 1 : 0, (int)combiner, op);
  });
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
  auto stream = current_hip_stream();
  const float* wptr =
      weights.defined() && weights.numel() ? weights.data_ptr<float>()
                                           : nullptr;
  dispatch_out_vec(out, dim, [&](auto* op, auto vec) {
    constexpr int VEC = decltype(vec)::value;
    using OutT = std::remove_pointer_t<decltype(op)>;
    k_group_pooled_fwd_q8<OutT, VEC>
        <<<n_blocks(batch * n_tables * (dim / VEC)), kBlock, 0, stream>>>(
            values.data_ptr<uint8_t>(), scales.data_ptr<float>(),
            default_values.data_ptr<float>(), keys.data_ptr<int64_t>(),
            slots.data_ptr<int32_t>(), inverse.data_ptr<int32_t>(),
            offsets.data_ptr<int32_t>(), wptr,
            combiner_ids.data_ptr<int32_t>(), (int)batch, (int)n_tables, dim,
            (int)(default_values.size(0) / n_tables), (int)key_bits,
            (float)no_permission_value, use_no_permission ? 1 : 0, op);
  });
  return out;
}

void register_quant_ev(py::module_& mod) {
  mod.def("ev_gather_q8", &ev_gather_q8);
  mod.def("seq_gather_pad_q8", &seq_gather_pad_q8);
  mod.def("pooled_fwd_q8", &pooled_fwd_q8);
  mod.def("group_pooled_fwd_q8", &group_pooled_fwd_q8);
}
