// ev_kernels.hip — MI355X (gfx950, CDNA4) embedding-engine kernels.
//
// The HBM embedding engine: an open-addressing (linear probe) hash table
// keyed by int64 feature id mapping to a monotonically-allocated int32
// value-slot, with per-entry frequency/version metadata for feature
// admission (counter filter) and eviction. Value rows live in a dense
// [max_slots, dim] fp32 slab; optimizer states are parallel slabs indexed
// by the same slots.
//
// Capability parity (not a port) with the reference engine:
//   - hash lookup/insert  ≙ GPUHashTable/cuco dynamic_map probing
//     (reference: gpu_hash_table.cu.cc:260-541) — re-designed as a single
//     flat power-of-two table with 64-wide-wavefront-friendly per-thread
//     probes; keys are pre-uniqued on the host side of the step so probes
//     are contention-free except first-insert CAS.
//   - fused gather+segment-pool ≙ EmbeddingLookUp + ApplyCombiner
//     (reference: fused_embedding_local_ops_gpu.cu.cc:42, SumUpEmbeddingShard)
//   - grad scatter ≙ DoEmbeddingGrad/DistributeGradToShard
//   - sparse optimizer applies ≙ training_ali_ops_gpu.cu.cc kernels,
//     operating directly on slot indices from the step's single probe
//     (the reference's `_OPT_` indices-as-pointers fusion); they live in
//     ev_apply_kernels.hip.
//
// CDNA4 notes: wavefront = 64; all elementwise kernels use a (row, dim)
// thread mapping with grid-stride so consecutive lanes read consecutive
// value-row elements (coalesced); blocks are multiples of 64; atomics are
// device-scope by default (per-XCD L2 non-coherence is safe).

#include "hip_common.h"

#define DEV_INLINE __device__ __forceinline__

static constexpr int64_t EMPTY_KEY = INT64_MIN;  // reserved sentinel
static constexpr int64_t PAD_KEY = INT64_MAX;    // wire-padding sentinel
static constexpr int kBlock = 256;

namespace {

DEV_INLINE uint64_t mix_hash(uint64_t k) {
  // splitmix64 finalizer — good avalanche for sequential ids
  k += 0x9E3779B97F4A7C15ull;
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  return k ^ (k >> 31);
}

DEV_INLINE float bf2f(__hip_bfloat16 v) { return __bfloat162float(v); }

// ---------------------------------------------------------------------
// hash probe / insert
// ---------------------------------------------------------------------

// Read-only linear probe: the entry index of `key`, or -1 when the probe
// reaches EMPTY_KEY (valid early exit: eviction compacts, no tombstones)
// or has wrapped the whole table.
DEV_INLINE int64_t ht_find(const int64_t* __restrict__ ht_keys,
                           int64_t cap_mask, int64_t key) {
  uint64_t h = mix_hash((uint64_t)key) & (uint64_t)cap_mask;
  for (int64_t probe = 0; probe <= cap_mask; ++probe) {
    int64_t idx = (int64_t)((h + probe) & (uint64_t)cap_mask);
    int64_t cur = ht_keys[idx];
    if (cur == key) return idx;
    if (cur == EMPTY_KEY) return -1;
  }
  return -1;
}

// Find `key` or claim (CAS) the first empty entry on its probe path; a
// fresh claim bumps entry_counter. Returns the entry index, or -1 when the
// table is full (host sizing bug: the caller raises error 2).
DEV_INLINE int64_t ht_find_or_claim(int64_t* __restrict__ ht_keys,
                                    int64_t cap_mask, int64_t key,
                                    int32_t* __restrict__ entry_counter) {
  uint64_t h = mix_hash((uint64_t)key) & (uint64_t)cap_mask;
  for (int64_t probe = 0; probe <= cap_mask; ++probe) {
    int64_t idx = (int64_t)((h + probe) & (uint64_t)cap_mask);
    int64_t cur = ht_keys[idx];
    if (cur != key) {
      if (cur != EMPTY_KEY) continue;
      int64_t prev = (int64_t)atomicCAS(
          (unsigned long long*)&ht_keys[idx],
          (unsigned long long)EMPTY_KEY, (unsigned long long)key);
      if (prev != EMPTY_KEY && prev != key) continue;  // lost race
      if (prev == EMPTY_KEY) atomicAdd(entry_counter, 1);
    }
    return idx;
  }
  return -1;
}

// Row of default_values that initializes `key`. Composite keys
// (EmbeddingCollection): table * dvd + (raw_key % dvd); key_bits == 0
// means plain keys.
DEV_INLINE int64_t default_row(int64_t key, int key_bits,
                               int default_value_dim) {
  if (key_bits > 0) {
    int64_t mask = ((int64_t)1 << key_bits) - 1;
    return (key >> key_bits) * default_value_dim +
           (int64_t)((uint64_t)(key & mask) % (uint64_t)default_value_dim);
  }
  return (int64_t)((uint64_t)key % (uint64_t)default_value_dim);
}

// Admit entry idx: grant a value slot and initialize its row from
// default_values. Returns the slot, or -1 with error 1 when the slab is
// out of space (host must grow).
DEV_INLINE int32_t ht_admit(
    int64_t key, int64_t idx, int32_t* __restrict__ ht_slot,
    int32_t* __restrict__ slot_counter, int max_slots,
    float* __restrict__ values, const float* __restrict__ default_values,
    int dim, int default_value_dim, int key_bits, int init_limit,
    int32_t* __restrict__ error_flag) {
  int32_t slot = atomicAdd(slot_counter, 1);
  if (slot >= max_slots) {
    atomicExch(error_flag, 1);
    return -1;
  }
  ht_slot[idx] = slot;
  // multi-tier (HBM_DRAM): rows at slot >= init_limit live in the host
  // cold slab; the host initializes those (kernel must not touch them)
  if (slot < init_limit) {
    const float* src =
        default_values + default_row(key, key_bits, default_value_dim) * dim;
    float* dst = values + (int64_t)slot * dim;
    for (int d = 0; d < dim; ++d) dst[d] = src[d];
  }
  return slot;
}

// Lookup-or-insert for a batch of UNIQUE keys. Per key:
//   - find or claim (CAS) a hash entry
//   - freq += count; version = step (no atomics needed: keys unique)
//   - admit a value slot once freq >= filter_freq; initialize the value
//     row from default_values[key % default_value_dim]
// out_slots[i] = slot or -1 (not admitted).
// NOTE every kernel whose grid n_blocks() caps at 65535 blocks MUST
// grid-stride: a plain `if (i >= n) return` silently dropped the tail of
// batches beyond 16.7M keys (found when a 120M-key rebalance rebuild
// lost most of the table).
__global__ void k_lookup_insert(
    const int64_t* __restrict__ keys, const int32_t* __restrict__ counts,
    int n, int64_t* __restrict__ ht_keys, int32_t* __restrict__ ht_slot,
    int32_t* __restrict__ ht_freq, int64_t* __restrict__ ht_version,
    int64_t cap_mask, int32_t* __restrict__ slot_counter,
    int32_t* __restrict__ entry_counter, int max_slots,
    float* __restrict__ values, const float* __restrict__ default_values,
    int dim, int default_value_dim, int key_bits, int init_limit,
    int filter_freq, int64_t step, int train,
    int32_t* __restrict__ out_slots, int32_t* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t gstride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += gstride) {
    const int64_t key = keys[i];
    int32_t slot = -1;
    if (!train) {
      int64_t idx = ht_find(ht_keys, cap_mask, key);
      if (idx >= 0) slot = ht_slot[idx];
    } else {
      int64_t idx = ht_find_or_claim(ht_keys, cap_mask, key, entry_counter);
      if (idx < 0) {
        atomicExch(error_flag, 2);  // table full (host sizing bug)
      } else {
        int32_t freq = ht_freq[idx] + (counts ? counts[i] : 1);
        ht_freq[idx] = freq;
        ht_version[idx] = step;
        slot = ht_slot[idx];
        if (slot < 0 && freq >= filter_freq)
          slot = ht_admit(key, idx, ht_slot, slot_counter, max_slots, values,
                          default_values, dim, default_value_dim, key_bits,
                          init_limit, error_flag);
      }
    }
    out_slots[i] = slot;
  }
}

// Bulk import used by restore: entries are created admitted with the given
// slot ids (slots pre-assigned densely by the host).
__global__ void k_insert_bulk(
    const int64_t* __restrict__ keys, const int32_t* __restrict__ slots,
    const int32_t* __restrict__ freqs, const int64_t* __restrict__ versions,
    int n, int64_t* __restrict__ ht_keys, int32_t* __restrict__ ht_slot,
    int32_t* __restrict__ ht_freq, int64_t* __restrict__ ht_version,
    int64_t cap_mask, int32_t* __restrict__ entry_counter,
    int32_t* __restrict__ error_flag) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t gstride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += gstride) {
    int64_t idx = ht_find_or_claim(ht_keys, cap_mask, keys[i], entry_counter);
    if (idx < 0) {
      atomicExch(error_flag, 2);
      continue;
    }
    ht_slot[idx] = slots[i];
    if (freqs) ht_freq[idx] = freqs[i];
    if (versions) ht_version[idx] = versions[i];
  }
}

// ---------------------------------------------------------------------
// fused hash dedup — replaces sort-based unique on the training hot path
// ---------------------------------------------------------------------
// The hash table itself deduplicates: pass A runs once per OCCURRENCE,
// inserting the key if absent and claiming a compact index [0, m) for the
// first toucher of this epoch (atomicExch on a per-entry epoch stamp —
// exactly one winner). Pass C (per occurrence) reads back inverse indices
// and exact per-batch counts. Pass B (per unique key) applies the
// frequency/version bookkeeping, admission + default-value init.
// Equivalent outputs to torch.unique(return_inverse, return_counts) + the
// probe, without any sort (the rocprim merge sorts were ~15% of the DLRM
// step).
//
// Scalars that advance per step (epoch, step, unique count) come either by
// value (eager path: the host knows them) or from a device scalar when its
// pointer is non-null (hipGraph capture: k_bump_epoch advances them inside
// the captured step, so replays keep deduplicating correctly with zero
// host involvement).

// SKIP_PAD (the padded sequence lookup): a PAD_KEY occurrence is not a key
// at all — no probe, no claim, no table entry; it records entry -1 for
// pass C (which skips it by key) and moves on. One body for both
// instantiations, so the claim logic cannot drift.
//
// MATRIX (the one-id-per-table layout): `keys` is the id matrix
// ids[batch, n_tables] itself, row-major, and occurrence j = t * batch + b
// has the composite key ids[b * n_tables + t] + (t << key_bits) — the
// table-major key array the collection would otherwise build with a
// transposing copy and an add. Reads are strided, the occ_entry write
// stays coalesced; pass A is bound by its table probes either way.
template <bool SKIP_PAD, bool MATRIX = false>
__global__ void k_dedup_pass_a(
    const int64_t* __restrict__ keys, int nnz, int64_t* __restrict__ ht_keys,
    int32_t* __restrict__ ht_epoch, int32_t* __restrict__ ht_compact,
    int64_t cap_mask, const int32_t* __restrict__ epoch_dev, int epoch_val,
    int32_t* __restrict__ entry_counter, int32_t* __restrict__ m_counter,
    int64_t* __restrict__ uniq_keys, int64_t* __restrict__ compact_entry,
    int64_t* __restrict__ occ_entry, int32_t* __restrict__ error_flag,
    int batch = 0, int n_tables = 0, int key_bits = 0) {
  const int epoch = epoch_dev ? *epoch_dev : epoch_val;
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) {
    int64_t key;
    if constexpr (MATRIX) {
      const int t = (int)j / batch;
      const int b = (int)j - t * batch;
      key = keys[(int64_t)b * n_tables + t] + ((int64_t)t << key_bits);
    } else {
      key = keys[j];
    }
    if constexpr (SKIP_PAD) {
      if (key == PAD_KEY) {
        occ_entry[j] = -1;
        continue;
      }
    }
    int64_t idx = ht_find_or_claim(ht_keys, cap_mask, key, entry_counter);
    if (idx < 0) {
      atomicExch(error_flag, 2);
      continue;
    }
    // freq/version updates live in pass B (one per UNIQUE key via pass
    // C's exact counts): hot keys were serializing thousands of
    // per-occurrence atomics on one cache line here. The plain read
    // short-circuits the epoch claim for already-claimed keys; racing
    // first-touchers are resolved by the atomicExch.
    if (ht_epoch[idx] != epoch) {
      int old = atomicExch(&ht_epoch[idx], epoch);
      if (old != epoch) {  // first toucher this step
        int c = atomicAdd(m_counter, 1);
        ht_compact[idx] = c;
        uniq_keys[c] = key;
        compact_entry[c] = idx;
      }
    }
    occ_entry[j] = idx;  // pass C reads compact ids WITHOUT re-probing
  }
}

__global__ void k_bump_epoch(int32_t* __restrict__ epoch_dev,
                             int64_t* __restrict__ step_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    epoch_dev[0] += 1;
    step_dev[0] += 1;
  }
}

// Prologue of a captured dedup, one launch for what were three: bump the
// epoch (and the step when step_dev is given, as k_bump_epoch does), zero
// the unique counter pass A claims from, and zero the n per-key counters
// pass C adds into. A kernel and not a memset for the reason k_zero_f32
// gives. Nothing here reads what it writes, so no ordering is needed
// inside the launch.
__global__ void k_dedup_begin(int32_t* __restrict__ epoch_dev,
                              int64_t* __restrict__ step_dev,
                              int32_t* __restrict__ m_counter,
                              int32_t* __restrict__ counts, int64_t n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    epoch_dev[0] += 1;
    if (step_dev) step_dev[0] += 1;
    m_counter[0] = 0;
    for (int64_t j = n & ~3LL; j < n; ++j) counts[j] = 0;
  }
  int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 4;
  int64_t stride = gridDim.x * (int64_t)blockDim.x * 4;
  for (; i + 3 < n; i += stride)
    *reinterpret_cast<int4*>(counts + i) = make_int4(0, 0, 0, 0);
}

// Pass B (per unique key): freq/version bookkeeping (one write per
// unique key, using pass C's exact per-batch counts — runs AFTER pass
// C), then admission + default-value init, slots out.
// Padded mode (m_dev non-null; hipGraph capture and the sharded exchange):
// the grid covers n = the nnz upper bound and the true unique count comes
// from the device counter, so no host sync happens inside the captured
// step. Tail entries get slot -1, and so does the wire-padding sentinel:
// no admission, no metadata (PAD_KEY's composite-decomposed default row
// would read far out of bounds of default_values).
__global__ void k_dedup_pass_b(
    const int64_t* __restrict__ compact_entry,
    const int64_t* __restrict__ uniq_keys, int n,
    const int32_t* __restrict__ m_dev, int32_t* __restrict__ ht_slot,
    int32_t* __restrict__ ht_freq, int64_t* __restrict__ ht_version,
    const int32_t* __restrict__ batch_counts,
    const int64_t* __restrict__ step_dev, int64_t step_val,
    int32_t* __restrict__ slot_counter, int max_slots,
    float* __restrict__ values, const float* __restrict__ default_values,
    int dim, int default_value_dim, int key_bits, int init_limit,
    int filter_freq, int32_t* __restrict__ out_slots,
    int32_t* __restrict__ error_flag) {
  const int m = m_dev ? *m_dev : n;
  const int64_t step = step_dev ? *step_dev : step_val;
  int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t gstride = gridDim.x * (int64_t)blockDim.x;
  for (; c < n; c += gstride) {
    if (m_dev && (c >= m || uniq_keys[c] == PAD_KEY)) {
      out_slots[c] = -1;
      continue;
    }
    int64_t idx = compact_entry[c];
    int32_t freq = ht_freq[idx] + batch_counts[c];
    ht_freq[idx] = freq;
    ht_version[idx] = step;
    int32_t slot = ht_slot[idx];
    if (slot < 0 && freq >= filter_freq)
      slot = ht_admit(uniq_keys[c], idx, ht_slot, slot_counter, max_slots,
                      values, default_values, dim, default_value_dim,
                      key_bits, init_limit, error_flag);
    out_slots[c] = slot;
  }
}

// Zero-fill (float4-wide). Used instead of hipMemsetAsync because memset
// nodes recorded during hipGraph capture were observed NOT to replay
// (counts/grad buffers accumulated across replays -> OOB scatters).
__global__ void k_zero_f32(float* __restrict__ p, int64_t n) {
  int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 4;
  int64_t stride = gridDim.x * (int64_t)blockDim.x * 4;
  for (; i + 3 < n; i += stride)
    *reinterpret_cast<float4*>(p + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t j = n & ~3LL; j < n; ++j) p[j] = 0.0f;
}

// ---------------------------------------------------------------------
// padded peer routing — the captured distributed exchange
// ---------------------------------------------------------------------
// The sharded collection's all-to-all must have static shapes to live
// inside a hipGraph (RCCL collectives capture, but only with fixed
// splits). Every peer slot is padded to `cap` rows; pad keys are
// PAD_KEY, which the owner deduplicates into one (ignored) entry, so no
// count exchange is needed on the wire at all (≙ the reference's
// two-phase count+payload protocol, all2all_input_dispatcher.cu:250-280,
// re-designed shape-static for graph replay).

// Bump only the dedup epoch (NOT the step): the distributed step runs
// TWO dedups per training step against the same table (requester-side
// claim-only dedup, then owner-side dedup of the padded exchange), and
// version/eviction semantics must advance once per step.
__global__ void k_bump_epoch_only(int32_t* __restrict__ epoch_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) epoch_dev[0] += 1;
}

// Reset the padded send layout: keys = PAD_KEY, counts = 0, cursors = 0.
__global__ void k_route_fill(int64_t* __restrict__ send_keys,
                             int32_t* __restrict__ send_cnt,
                             int32_t* __restrict__ peer_cursor, int total,
                             int world) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < total; i += stride) {
    send_keys[i] = PAD_KEY;
    send_cnt[i] = 0;
    if (i < world) peer_cursor[i] = 0;
  }
}

// Scatter the step's unique keys into per-peer padded blocks.
// owner = (key & key_mask) % world (the raw id routes; composite table
// tags are stripped). route_pos[u] remembers where unique u landed so
// the returned embedding rows / outgoing grad rows can be addressed
// without any host-side ordering. Overflowing a peer's cap sets
// error_flag = 4 (host must re-capture with a larger cap).
//
// Cursor reservation is BLOCK-AGGREGATED: per-owner counts collect in
// LDS (fast bank atomics), then one global atomicAdd per (block, owner)
// reserves a range. A naive per-element global atomic serialized on the
// per-owner cache line (measured 525 us at world=1; this form is ~30 us).
static constexpr int kMaxWorld = 64;

__global__ void k_route_pad(
    const int64_t* __restrict__ uniq_keys, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ m_dev, int n_cap, int world, int cap,
    int key_bits, int64_t* __restrict__ send_keys,
    int32_t* __restrict__ send_cnt, int32_t* __restrict__ route_pos,
    int32_t* __restrict__ peer_cursor, int32_t* __restrict__ error_flag) {
  const int m = min(*m_dev, n_cap);
  const int64_t key_mask =
      key_bits > 0 ? (((int64_t)1 << key_bits) - 1) : ~(int64_t)0;
  __shared__ int32_t lcnt[kMaxWorld];
  __shared__ int32_t lbase[kMaxWorld];
  // grid-stride by whole blocks so every thread of a block participates
  // in the aggregation barriers
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < m;
       base += (int64_t)gridDim.x * blockDim.x) {
    int64_t u = base + threadIdx.x;
    for (int o = threadIdx.x; o < world; o += blockDim.x) lcnt[o] = 0;
    __syncthreads();
    int owner = -1, my = 0;
    int64_t key = 0;
    if (u < m) {
      key = uniq_keys[u];
      owner = (int)((uint64_t)(key & key_mask) % (uint64_t)world);
      my = atomicAdd(&lcnt[owner], 1);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < world; o += blockDim.x)
      lbase[o] = lcnt[o] ? atomicAdd(&peer_cursor[o], lcnt[o]) : 0;
    __syncthreads();
    if (u < m) {
      int pos = lbase[owner] + my;
      if (pos >= cap) {
        atomicExch(error_flag, 4);
        route_pos[u] = owner * cap;  // in-bounds dummy; run is poisoned
      } else {
        int64_t o = (int64_t)owner * cap + pos;
        send_keys[o] = key;
        send_cnt[o] = counts[u];
        route_pos[u] = (int32_t)o;
      }
    }
    __syncthreads();
  }
}

// Owner-side helpers, PAD-aware. The pads are the scaling hazard: every
// pad element maps to ONE unique (PAD_KEY), so generic index_add /
// counting kernels serialize hundreds of thousands of atomics on a
// single cache line (measured: torch index_add 783 us/step, pass C
// 161 us). Pass C (given keys) and all kernels below skip pad elements
// outright.

// slots_elem[j] = inverse[j] < 0 ? -1 : slots[inverse[j]]
// (replaces a .long() cast + index_select pair)
__global__ void k_slots_gather_pad(const int32_t* __restrict__ inverse,
                                   const int32_t* __restrict__ slots,
                                   int nnz, int32_t* __restrict__ out) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) {
    int c = inverse[j];
    out[j] = c < 0 ? -1 : slots[c];
  }
}

// cnt_sum[inverse[j]] += cnt[j] for non-pad elements. A unique key
// repeats at most `world` times here (peers), so atomic contention is
// bounded by the world size.
__global__ void k_cnt_sum_pad(const int32_t* __restrict__ inverse,
                              const int32_t* __restrict__ cnt, int nnz,
                              int32_t* __restrict__ cnt_sum) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) {
    int c = inverse[j];
    if (c >= 0) atomicAdd(&cnt_sum[c], cnt[j]);
  }
}

// grad2[inverse[j]] += grad[j] rows for non-pad elements (the owner-side
// cross-peer gradient reduction; <= world-way contention per row).
__global__ void k_rows_segsum_pad(const float* __restrict__ grad,
                                  const int32_t* __restrict__ inverse,
                                  int nnz, int dim,
                                  float* __restrict__ grad2) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = (int64_t)nnz * dim;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    int j = (int)(t / dim);
    int c = inverse[j];
    if (c < 0) continue;
    int d = (int)(t % dim);
    atomicAdd(&grad2[(int64_t)c * dim + d], grad[t]);
  }
}

// inv_out[j] = lut[inv_in[j]] — composes the requester inverse with the
// routed positions in one pass (no int64 cast round trip).
__global__ void k_compose_i32(const int32_t* __restrict__ inv_in,
                              const int32_t* __restrict__ lut, int nnz,
                              int32_t* __restrict__ inv_out) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) inv_out[j] = lut[inv_in[j]];
}

// dst[route_pos[u]] = src[u] for u < m (grad rows into the padded wire
// layout; dst is pre-zeroed so pad rows carry zero gradient).
__global__ void k_rows_to_padded(const float* __restrict__ src,
                                 const int32_t* __restrict__ route_pos,
                                 const int32_t* __restrict__ m_dev,
                                 int n_cap, int dim,
                                 float* __restrict__ dst) {
  const int m = min(*m_dev, n_cap);
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = (int64_t)m * dim;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    int u = (int)(t / dim);
    int d = (int)(t % dim);
    dst[(int64_t)route_pos[u] * dim + d] = src[t];
  }
}

// Wave-level grouping of equal values: zipf-hot keys put many equal keys
// into one wave (the hottest DLRM key fills ~19 of 64 lanes of every wave
// of its table), and per-occurrence atomics on them form one serial chain
// per key. Pass C merges a wave's duplicates in registers and lets one
// leader lane per distinct value touch memory.
struct WaveGroup {
  uint64_t mask;  // valid lanes of this wave holding the same value
  int leader;     // lowest lane of mask
  int pos;        // this lane's position inside mask
};

// Registers only (ballots and one shuffle per 8 rounds, no memory
// operation). Must be called by the WHOLE wave, converged; lanes with
// valid == false get mask 0 / leader 0 / pos 0.
//
// One ballot per value BIT splits the lanes into classes agreeing on the
// bits seen so far. Classes only ever split, and equal values share every
// bit, so as soon as every lane equals the lowest lane of its class the
// classes are exactly the groups of equal values. With values whose low
// bits are spread (hash-table entries) that holds after ~2*log2(64) bits
// whether the wave holds 64 distinct values or one hot one; a loop that
// retires one distinct value per round needs 64 rounds on all-distinct
// input, which doubled pass C's time there.
DEV_INLINE WaveGroup wave_group_by(uint64_t v, bool valid) {
  WaveGroup g{0ull, 0, 0};
  const int lane = __lane_id();
  uint64_t mask = __ballot(valid);
  int leader = lane;
  for (int b = 0; b < 64; b += 8) {  // wave-uniform trip count
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool bit = (v >> (b + i)) & 1ull;
      const uint64_t with = __ballot(bit);
      mask &= bit ? with : ~with;  // a valid lane always keeps its own bit
    }
    leader = valid ? __ffsll((unsigned long long)mask) - 1 : lane;
    const uint64_t lv = __shfl(v, leader);
    if (!__ballot(valid && lv != v)) break;  // every class is one value
  }
  if (valid) {
    g.mask = mask;
    g.leader = leader;
    g.pos = __popcll(mask & ((1ull << lane) - 1ull));
  }
  return g;
}

// First element of this wave's 64-wide slice and the grid's slice stride,
// both wave-uniform, so a caller's grid-stride loop keeps every lane of the
// wave in the loop (tail lanes are predicated, never exit early).
DEV_INLINE int64_t wave_slice_begin() {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  return (blockIdx.x * (int64_t)(blockDim.x >> 6) + wave) * 64;
}
DEV_INLINE int64_t wave_slice_stride() {
  return gridDim.x * (int64_t)(blockDim.x >> 6) * 64;
}

// Pass C (per occurrence): inverse + exact per-batch counts. Index-direct:
// pass A recorded each occurrence's hash entry, so inverse/rank need NO
// re-probe of the table (the probe was ~half of the dedup cost at 213k
// occurrences over a 16M-entry table). With `keys` given (owner side of
// the sharded exchange) PAD_KEY elements get inverse -1 / rank 0 and
// touch no counter.
__global__ void k_dedup_pass_c(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ occ_entry,
    int nnz, const int32_t* __restrict__ ht_compact,
    int32_t* __restrict__ inverse, int32_t* __restrict__ counts,
    int32_t* __restrict__ rank) {
  const int lane = __lane_id();
  const int64_t stride = wave_slice_stride();
  for (int64_t j0 = wave_slice_begin(); j0 < nnz; j0 += stride) {
    const int64_t j = j0 + lane;
    const bool in_range = j < nnz;
    const bool valid = in_range && !(keys && keys[j] == PAD_KEY);
    const int64_t entry = valid ? occ_entry[j] : 0;
    // a wave's occurrences of one key share ONE returning atomic (a hot
    // key's per-occurrence adds were a serial chain on one word); all
    // leaders of the wave issue theirs in the same instruction
    const WaveGroup g = wave_group_by((uint64_t)entry, valid);
    int c = -1, base = 0;
    if (valid && lane == g.leader) {
      c = ht_compact[entry];
      base = atomicAdd(&counts[c], __popcll(g.mask));
    }
    c = __shfl(c, g.leader);
    base = __shfl(base, g.leader);
    if (in_range) {
      inverse[j] = valid ? c : -1;
      // the counter value doubles as this occurrence's rank within its
      // key, letting the CSR order build become a direct scatter
      // (k_csr_scatter) instead of a second atomic-cursor pass
      rank[j] = valid ? base + g.pos : 0;
    }
  }
}

// CSR bounds: bounds[0] = 0, bounds[i + 1] = counts[0] + ... + counts[i],
// int32 throughout, in two launches. k_tile_sums writes one total per tile
// of kScanTile counts; k_csr_bounds then has each block add up the tile
// totals in front of its tile and scan the tile itself. No block ever
// waits for another (no look-back, no flags): the only dependency is the
// kernel boundary. Both grid-stride over tiles, so the grid cap
// (kScanMaxBlocks) bounds nothing but parallelism.
constexpr int kScanPer = 4;
constexpr int kScanTile = kBlock * kScanPer;
constexpr int kScanMaxBlocks = 1024;

// Sum of v over the block, returned to every thread. `red` holds kBlock
// ints; two barriers, so back-to-back calls may reuse it.
DEV_INLINE int block_sum_i32(int v, int* __restrict__ red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const int total = red[0];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kBlock) void k_tile_sums(
    const int32_t* __restrict__ counts, int64_t m, int n_tiles,
    int32_t* __restrict__ tile_sums) {
  __shared__ int red[kBlock];
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t i0 = (int64_t)t * kScanTile + threadIdx.x * kScanPer;
    int v = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k)
      if (i0 + k < m) v += counts[i0 + k];
    const int total = block_sum_i32(v, red);
    if (threadIdx.x == 0) tile_sums[t] = total;
  }
}

__global__ __launch_bounds__(kBlock) void k_csr_bounds(
    const int32_t* __restrict__ counts, int64_t m, int n_tiles,
    const int32_t* __restrict__ tile_sums, int32_t* __restrict__ bounds) {
  __shared__ int red[kBlock];
  __shared__ int scan[2][kBlock];
  if (blockIdx.x == 0 && threadIdx.x == 0) bounds[0] = 0;
  int base = 0;   // sum of the tile totals in [0, summed)
  int summed = 0;
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    int part = 0;
    for (int u = summed + threadIdx.x; u < t; u += kBlock)
      part += tile_sums[u];
    base += block_sum_i32(part, red);
    summed = t;
    const int64_t i0 = (int64_t)t * kScanTile + threadIdx.x * kScanPer;
    int c[kScanPer];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      c[k] = i0 + k < m ? counts[i0 + k] : 0;
      mine += c[k];
    }
    // inclusive Hillis-Steele scan of the per-thread totals
    int cur = 0;
    scan[0][threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
      int v = scan[cur][threadIdx.x];
      if ((int)threadIdx.x >= d) v += scan[cur][threadIdx.x - d];
      scan[cur ^ 1][threadIdx.x] = v;
      cur ^= 1;
      __syncthreads();
    }
    int run = base + scan[cur][threadIdx.x] - mine;
    __syncthreads();  // scan[] is rewritten by the next tile
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      run += c[k];
      if (i0 + k < m) bounds[i0 + k + 1] = run;
    }
  }
}

// order[bounds[c] + rank[j]] = j — direct scatter using pass C's ranks.
// The destination is bounds-guarded: a corrupt inverse/rank pair (e.g. a
// key pass C failed to find) must trip the error flag, not fault the GPU.
__global__ void k_csr_scatter(const int32_t* __restrict__ inverse,
                              const int32_t* __restrict__ rank, int nnz,
                              const int32_t* __restrict__ bounds,
                              int32_t* __restrict__ order,
                              int32_t* __restrict__ error_flag) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) {
    int64_t o = (int64_t)bounds[inverse[j]] + rank[j];
    if (o < 0 || o >= nnz) {
      atomicExch(error_flag, 3);
      continue;
    }
    order[o] = (int32_t)j;
  }
}

// Fill n int32 words with v. A kernel for the reason k_zero_f32 gives:
// memset nodes did not replay under hipGraph capture.
__global__ void k_fill_i32(int32_t* __restrict__ p, int64_t n, int32_t v) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// k_csr_scatter over a padded stream: occurrences with inverse < 0 (pads)
// are not part of any key's run and are skipped, so `order` (pre-filled
// with -1) lists the valid occurrences in [0, n_valid) and -1 after. m is
// the number of rows of `bounds` minus one; an inverse past it, or a
// destination outside order, trips error 3 instead of being dereferenced.
__global__ void k_csr_scatter_pad(const int32_t* __restrict__ inverse,
                                  const int32_t* __restrict__ rank, int nnz,
                                  const int32_t* __restrict__ bounds, int m,
                                  int32_t* __restrict__ order,
                                  int32_t* __restrict__ error_flag) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) {
    const int c = inverse[j];
    if (c < 0) continue;
    if (c >= m) {
      atomicExch(error_flag, 3);
      continue;
    }
    int64_t o = (int64_t)bounds[c] + rank[j];
    if (o < 0 || o >= nnz) {
      atomicExch(error_flag, 3);
      continue;
    }
    order[o] = (int32_t)j;
  }
}

// CSR order build: order[bounds[c] + pos++] = j (pos via per-key cursor).
__global__ void k_csr_order(const int32_t* __restrict__ inverse, int nnz,
                            const int32_t* __restrict__ bounds,
                            int32_t* __restrict__ cursor,
                            int32_t* __restrict__ order) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; j < nnz; j += stride) {
    int c = inverse[j];
    int pos = atomicAdd(&cursor[c], 1);
    order[bounds[c] + pos] = (int32_t)j;
  }
}

// Zero-copy gather of cold-tier rows: the GPU dereferences pinned host
// memory directly (unified addressing), so the multi-tier staging path
// (≙ CopyEmbeddingsFromDramToHbm, hbm_dram_storage.h:412-435) is ONE
// kernel at interconnect bandwidth instead of a single-threaded CPU
// gather + copy (measured 0.4 GB/s on the CPU path).
__global__ void k_gather_host_rows(const float* __restrict__ host_src,
                                   const int64_t* __restrict__ rows,
                                   int64_t m, int dim,
                                   float* __restrict__ out) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = m * dim;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride)
    out[t] = host_src[rows[t / dim] * dim + t % dim];
}

// Reverse direction: scatter updated rows back into the pinned cold slab
// (cold-tier optimizer writes).
__global__ void k_scatter_host_rows(const float* __restrict__ src,
                                    const int64_t* __restrict__ rows,
                                    int64_t m, int dim,
                                    float* __restrict__ host_dst) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = m * dim;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride)
    host_dst[rows[t / dim] * dim + t % dim] = src[t];
}

// Read-only probe (serving / frequency / version queries).
// out_slots: slot or -1; out_entry: hash index or -1 (metadata access).
__global__ void k_lookup(
    const int64_t* __restrict__ keys, int n,
    const int64_t* __restrict__ ht_keys, const int32_t* __restrict__ ht_slot,
    int64_t cap_mask, int32_t* __restrict__ out_slots,
    int64_t* __restrict__ out_entry) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t gstride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += gstride) {
    int64_t idx = ht_find(ht_keys, cap_mask, keys[i]);
    out_slots[i] = idx >= 0 ? ht_slot[idx] : -1;
    if (out_entry) out_entry[i] = idx;
  }
}

// Export scan: compact live hash entries into dense output arrays.
__global__ void k_export_scan(
    const int64_t* __restrict__ ht_keys, const int32_t* __restrict__ ht_slot,
    const int32_t* __restrict__ ht_freq,
    const int64_t* __restrict__ ht_version, int64_t capacity,
    int32_t* __restrict__ cursor, int64_t* __restrict__ out_keys,
    int32_t* __restrict__ out_slots, int32_t* __restrict__ out_freqs,
    int64_t* __restrict__ out_versions, int out_cap) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < capacity; i += stride) {
    int64_t k = ht_keys[i];
    if (k == EMPTY_KEY) continue;
    int32_t pos = atomicAdd(cursor, 1);
    if (pos >= out_cap) continue;
    out_keys[pos] = k;
    out_slots[pos] = ht_slot[i];
    out_freqs[pos] = ht_freq[i];
    out_versions[pos] = ht_version[i];
  }
}

// ---------------------------------------------------------------------
// pooled backward (the forward read kernels are in ev_read_kernels.hip)
// ---------------------------------------------------------------------

// Pooled backward: grad_unique[u][d] += coeff(b) * w_j * grad_out[b][d]
// for every occurrence j of unique key u. Thread = (b, d); atomicAdd into
// grad_unique (unique keys repeat across rows).
template <typename GradT>
__global__ void k_pooled_bwd(
    const GradT* __restrict__ grad_out, const int32_t* __restrict__ inverse,
    const int32_t* __restrict__ offsets, const float* __restrict__ weights,
    int batch, int dim, int combiner, float* __restrict__ grad_unique) {
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t total = (int64_t)batch * dim;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; t < total; t += stride) {
    int b = (int)(t / dim);
    int d = (int)(t % dim);
    int beg = offsets[b], end = offsets[b + 1];
    int len = end - beg;
    if (len == 0) continue;
    float g;
    if constexpr (std::is_same_v<GradT, __hip_bfloat16>) g = bf2f(grad_out[t]);
    else g = grad_out[t];
    float coeff = 1.0f;
    if (combiner != 0) {
      float wacc = 0.0f;
      if (weights) {
        for (int j = beg; j < end; ++j)
          wacc += (combiner == 2) ? weights[j] * weights[j] : weights[j];
      } else {
        wacc = (float)len;
      }
      float denom = (combiner == 2) ? sqrtf(wacc) : wacc;
      coeff = denom > 1e-12f ? 1.0f / denom : 0.0f;
    }
    float gc = g * coeff;
    for (int j = beg; j < end; ++j) {
      float w = weights ? weights[j] : 1.0f;
      atomicAdd(&grad_unique[(int64_t)inverse[j] * dim + d], w * gc);
    }
  }
}

// ---------------------------------------------------------------------
// grouped (multi-table) pooled backward — the EmbeddingCollection hot path
// ---------------------------------------------------------------------
//
// N tables of equal dim share one storage via composite keys
// (table_id << key_bits) | id. One unique + one probe + one fused kernel
// per step regardless of table count (reference capability:
// GroupEmbeddingVarLookup, ops/kv_variable_ops.cc:404, re-designed so the
// whole group is ONE launch instead of one block-set per table).
//
// Ragged layout: the N tables' ragged batches are concatenated —
// offsets[(N*B)+1]; pooled row r (< N*B) is table t = r / B, sample
// b = r % B. The forward (k_group_pooled_fwd, ev_read_kernels.hip) writes
// its output interleaved as out[b, t*D + d], the [B, N*D] concat layout
// models consume with no extra copy; grad_out arrives in that layout.

// Balanced segmented grad scatter. Work is split over OCCURRENCES in
// sorted (CSR) order, not over unique keys: a group of LANES lanes (one
// lane per embedding column, d += LANES for wider rows) owns R consecutive
// positions k of `order`, so work per thread is constant whatever the key
// skew and nothing runs for padded unique rows. All R gradient loads are
// issued before the first add; runs of equal u = inverse[order[k]] are
// summed in registers. A run that lies wholly inside the group (checked
// against the neighbouring positions' u) stores plainly; a run cut by a
// group edge adds atomically into the zero-filled output.
// IDENTITY: the matrix fast path (one id per table per sample) has
// row_ids == arange and unit combiner coefficients — skip both reads.
// Corrupt indices (order/inverse/row id out of range) are skipped, never
// dereferenced.
template <typename GradT, int LANES, int R, bool IDENTITY>
__global__ void k_group_pooled_bwd_seg(
    const GradT* __restrict__ grad_out, const int32_t* __restrict__ order,
    const int32_t* __restrict__ inverse, const int32_t* __restrict__ row_ids,
    const float* __restrict__ weights, const float* __restrict__ row_coeff,
    int nnz, int m_rows, int batch, int n_tables, int dim,
    float* __restrict__ grad_unique) {
  constexpr int kGroups = kBlock / LANES;  // groups per block
  const int l = threadIdx.x % LANES;
  const int64_t step = gridDim.x * (int64_t)kGroups * R;
  const int n_rows = batch * n_tables;
  auto u_at = [&](int64_t k) -> int {
    if (k < 0 || k >= nnz) return -2;
    int j = order[k];
    if ((unsigned)j >= (unsigned)nnz) return -1;
    int u = inverse[j];
    return (unsigned)u < (unsigned)m_rows ? u : -1;
  };
  for (int64_t k0 = (blockIdx.x * (int64_t)kGroups + threadIdx.x / LANES) * R;
       k0 < nnz; k0 += step) {
    int u[R], grow[R];
    float cf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      u[r] = -2;
      grow[r] = 0;
      cf[r] = 1.0f;
      const int64_t k = k0 + r;
      if (k < nnz) {
        const int j = order[k];
        if ((unsigned)j >= (unsigned)nnz) { u[r] = -1; continue; }
        const int rid = IDENTITY ? j : row_ids[j];
        const int uu = inverse[j];
        if ((unsigned)uu >= (unsigned)m_rows ||
            (unsigned)rid >= (unsigned)n_rows) { u[r] = -1; continue; }
        u[r] = uu;
        grow[r] = (rid % batch) * n_tables + rid / batch;
        if constexpr (!IDENTITY)
          cf[r] = (weights ? weights[j] : 1.0f) * row_coeff[rid];
      }
    }
    const int u_prev = u_at(k0 - 1);
    const int u_next = u_at(k0 + R);
    for (int d = l; d < dim; d += LANES) {
      float g[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        g[r] = 0.0f;
        if (u[r] >= 0) {
          const int64_t gidx = (int64_t)grow[r] * dim + d;
          if constexpr (std::is_same_v<GradT, __hip_bfloat16>)
            g[r] = bf2f(grad_out[gidx]);
          else
            g[r] = grad_out[gidx];
        }
      }
      float acc = 0.0f;
      bool cut = u[0] >= 0 && u_prev == u[0];  // run began in the group before
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (u[r] < 0) continue;
        if constexpr (IDENTITY) acc += g[r];
        else acc += cf[r] * g[r];
        const int un = (r + 1 < R) ? u[r + 1] : u_next;
        if (un == u[r] && r + 1 < R) continue;  // run goes on in this group
        float* dst = &grad_unique[(int64_t)u[r] * dim + d];
        if (cut || un == u[r]) atomicAdd(dst, acc);
        else *dst = acc;
        acc = 0.0f;
        cut = false;
      }
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")

// Zero n 4-byte words (fp32 or int32) on the stream; see k_zero_f32 for
// why this is not hipMemsetAsync.
static inline void zero_fill(void* p, int64_t n, hipStream_t stream) {
  if (n <= 0) return;  // an empty grid is a launch error
  k_zero_f32<<<n_blocks((n + 3) / 4), kBlock, 0, stream>>>(
      static_cast<float*>(p), n);
}

torch::Tensor ht_lookup_insert(
    torch::Tensor keys, torch::Tensor counts, torch::Tensor ht_keys,
    torch::Tensor ht_slot, torch::Tensor ht_freq, torch::Tensor ht_version,
    torch::Tensor slot_counter, torch::Tensor entry_counter,
    torch::Tensor values, torch::Tensor default_values, int64_t max_slots,
    int64_t dvd_per_table, int64_t key_bits, int64_t init_limit,
    int64_t filter_freq, int64_t step, bool train,
    torch::Tensor error_flag) {
  CHECK_DEV(keys);
  int n = keys.numel();
  auto out = torch::empty({n}, keys.options().dtype(torch::kInt32));
  if (n == 0) return out;
  auto stream = current_hip_stream();
  int dim = values.size(1);
  k_lookup_insert<<<n_blocks(n), kBlock, 0, stream>>>(
      keys.data_ptr<int64_t>(),
      counts.defined() && counts.numel() ? counts.data_ptr<int32_t>()
                                         : nullptr,
      n, ht_keys.data_ptr<int64_t>(), ht_slot.data_ptr<int32_t>(),
      ht_freq.data_ptr<int32_t>(), ht_version.data_ptr<int64_t>(),
      ht_keys.numel() - 1, slot_counter.data_ptr<int32_t>(),
      entry_counter.data_ptr<int32_t>(), (int)max_slots,
      values.data_ptr<float>(), default_values.data_ptr<float>(), dim,
      (int)dvd_per_table, (int)key_bits, (int)init_limit, (int)filter_freq,
      step, train ? 1 : 0, out.data_ptr<int32_t>(),
      error_flag.data_ptr<int32_t>());
  return out;
}

// The dedup passes take each per-step scalar (epoch, step, unique count)
// either from a device scalar (hipGraph capture) or by value when the
// optional tensor is None (eager: the host knows it).
template <typename T>
static inline const T* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr<T>() : nullptr;
}

template <bool SKIP_PAD, bool MATRIX = false>
static torch::Tensor dedup_a_impl(
    torch::Tensor keys, torch::Tensor ht_keys, torch::Tensor ht_epoch,
    torch::Tensor ht_compact, c10::optional<torch::Tensor> epoch_dev,
    int64_t epoch, torch::Tensor entry_counter, torch::Tensor m_counter,
    torch::Tensor uniq_keys, torch::Tensor compact_entry,
    torch::Tensor occ_entry, torch::Tensor error_flag, int batch = 0,
    int n_tables = 0, int key_bits = 0) {
  int64_t nnz = keys.numel();
  if (nnz == 0) return m_counter;
  auto stream = current_hip_stream();
  k_dedup_pass_a<SKIP_PAD, MATRIX><<<n_blocks(nnz), kBlock, 0, stream>>>(
      keys.data_ptr<int64_t>(), (int)nnz, ht_keys.data_ptr<int64_t>(),
      ht_epoch.data_ptr<int32_t>(), ht_compact.data_ptr<int32_t>(),
      ht_keys.numel() - 1, opt_ptr<int32_t>(epoch_dev), (int)epoch,
      entry_counter.data_ptr<int32_t>(), m_counter.data_ptr<int32_t>(),
      uniq_keys.data_ptr<int64_t>(), compact_entry.data_ptr<int64_t>(),
      occ_entry.data_ptr<int64_t>(), error_flag.data_ptr<int32_t>(), batch,
      n_tables, key_bits);
  return m_counter;
}

torch::Tensor ht_dedup_a(torch::Tensor keys, torch::Tensor ht_keys,
                         torch::Tensor ht_epoch, torch::Tensor ht_compact,
                         c10::optional<torch::Tensor> epoch_dev,
                         int64_t epoch, torch::Tensor entry_counter,
                         torch::Tensor m_counter, torch::Tensor uniq_keys,
                         torch::Tensor compact_entry,
                         torch::Tensor occ_entry, torch::Tensor error_flag) {
  return dedup_a_impl<false>(keys, ht_keys, ht_epoch, ht_compact, epoch_dev,
                             epoch, entry_counter, m_counter, uniq_keys,
                             compact_entry, occ_entry, error_flag);
}

// Pass A of the padded sequence lookup: PAD_KEY occurrences touch nothing
// and get occ_entry -1 (pair it with ht_dedup_c(keys=...)).
torch::Tensor ht_dedup_a_pad(torch::Tensor keys, torch::Tensor ht_keys,
                             torch::Tensor ht_epoch, torch::Tensor ht_compact,
                             c10::optional<torch::Tensor> epoch_dev,
                             int64_t epoch, torch::Tensor entry_counter,
                             torch::Tensor m_counter, torch::Tensor uniq_keys,
                             torch::Tensor compact_entry,
                             torch::Tensor occ_entry,
                             torch::Tensor error_flag) {
  return dedup_a_impl<true>(keys, ht_keys, ht_epoch, ht_compact, epoch_dev,
                            epoch, entry_counter, m_counter, uniq_keys,
                            compact_entry, occ_entry, error_flag);
}

// Pass A straight from the id matrix ids[batch, n_tables] (int64,
// contiguous): occurrence t * batch + b is ids[b, t] + (t << key_bits), the
// order EmbeddingCollection.matrix_inputs builds, without building it.
torch::Tensor ht_dedup_a_matrix(
    torch::Tensor ids, int64_t key_bits, torch::Tensor ht_keys,
    torch::Tensor ht_epoch, torch::Tensor ht_compact,
    c10::optional<torch::Tensor> epoch_dev, int64_t epoch,
    torch::Tensor entry_counter, torch::Tensor m_counter,
    torch::Tensor uniq_keys, torch::Tensor compact_entry,
    torch::Tensor occ_entry, torch::Tensor error_flag) {
  CHECK_DEV(ids);
  TORCH_CHECK(ids.dim() == 2 && ids.is_contiguous() &&
                  ids.scalar_type() == torch::kInt64,
              "ht_dedup_a_matrix: ids must be contiguous int64 [batch, n]");
  TORCH_CHECK(ids.numel() <= INT32_MAX, "ht_dedup_a_matrix: too many ids");
  TORCH_CHECK(key_bits > 0 && key_bits < 63 &&
                  ids.size(1) <= ((int64_t)1 << (63 - key_bits)),
              "ht_dedup_a_matrix: table tag does not fit above key_bits");
  TORCH_CHECK(uniq_keys.numel() >= ids.numel() &&
                  compact_entry.numel() >= ids.numel() &&
                  occ_entry.numel() >= ids.numel(),
              "ht_dedup_a_matrix: output buffers are smaller than ids");
  return dedup_a_impl<false, true>(
      ids, ht_keys, ht_epoch, ht_compact, epoch_dev, epoch, entry_counter,
      m_counter, uniq_keys, compact_entry, occ_entry, error_flag,
      (int)ids.size(0), (int)ids.size(1), (int)key_bits);
}

torch::Tensor ht_dedup_b(torch::Tensor compact_entry, torch::Tensor uniq_keys,
                         c10::optional<torch::Tensor> m_dev,
                         torch::Tensor ht_slot, torch::Tensor ht_freq,
                         torch::Tensor ht_version,
                         torch::Tensor batch_counts,
                         c10::optional<torch::Tensor> step_dev, int64_t step,
                         torch::Tensor slot_counter, int64_t max_slots,
                         torch::Tensor values, torch::Tensor default_values,
                         int64_t dvd_per_table, int64_t key_bits,
                         int64_t init_limit, int64_t filter_freq,
                         torch::Tensor error_flag) {
  int n = uniq_keys.numel();
  auto slots = torch::empty({n}, ht_slot.options());
  if (n == 0) return slots;
  auto stream = current_hip_stream();
  k_dedup_pass_b<<<n_blocks(n), kBlock, 0, stream>>>(
      compact_entry.data_ptr<int64_t>(), uniq_keys.data_ptr<int64_t>(), n,
      opt_ptr<int32_t>(m_dev), ht_slot.data_ptr<int32_t>(),
      ht_freq.data_ptr<int32_t>(), ht_version.data_ptr<int64_t>(),
      batch_counts.data_ptr<int32_t>(), opt_ptr<int64_t>(step_dev), step,
      slot_counter.data_ptr<int32_t>(), (int)max_slots,
      values.data_ptr<float>(), default_values.data_ptr<float>(),
      values.size(1), (int)dvd_per_table, (int)key_bits, (int)init_limit,
      (int)filter_freq, slots.data_ptr<int32_t>(),
      error_flag.data_ptr<int32_t>());
  return slots;
}

void bump_epoch(torch::Tensor epoch_dev, torch::Tensor step_dev) {
  k_bump_epoch<<<1, 64, 0, current_hip_stream()>>>(
      epoch_dev.data_ptr<int32_t>(), step_dev.data_ptr<int64_t>());
}

void bump_epoch_only(torch::Tensor epoch_dev) {
  k_bump_epoch_only<<<1, 64, 0, current_hip_stream()>>>(
      epoch_dev.data_ptr<int32_t>());
}

// step_dev None: epoch only (a second lookup within one step).
void dedup_begin(torch::Tensor epoch_dev,
                 c10::optional<torch::Tensor> step_dev,
                 torch::Tensor m_counter, torch::Tensor counts) {
  CHECK_DEV(counts);
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 &&
                  counts.is_contiguous() &&
                  m_counter.scalar_type() == torch::kInt32 &&
                  m_counter.numel() == 1,
              "dedup_begin: counts int32 contiguous, m_counter int32 [1]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(counts.data_ptr()) % 16 == 0,
              "dedup_begin: counts must be 16-byte aligned");
  const int64_t n = counts.numel();
  k_dedup_begin<<<std::max(1, n_blocks((n + 3) / 4)), kBlock, 0,
                  current_hip_stream()>>>(
      epoch_dev.data_ptr<int32_t>(),
      step_dev.has_value() ? step_dev->data_ptr<int64_t>() : nullptr,
      m_counter.data_ptr<int32_t>(), counts.data_ptr<int32_t>(), n);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> route_pad(
    torch::Tensor uniq_keys, torch::Tensor counts, torch::Tensor m_dev,
    int64_t world, int64_t cap, int64_t key_bits,
    torch::Tensor error_flag) {
  int n_cap = uniq_keys.numel();
  int total = (int)(world * cap);
  auto opts_i32 = counts.options();
  auto send_keys = torch::empty({(int64_t)total}, uniq_keys.options());
  auto send_cnt = torch::empty({(int64_t)total}, opts_i32);
  auto route_pos = torch::empty({(int64_t)n_cap}, opts_i32);
  auto cursor = torch::empty({world}, opts_i32);
  auto stream = current_hip_stream();
  k_route_fill<<<n_blocks(total), kBlock, 0, stream>>>(
      send_keys.data_ptr<int64_t>(), send_cnt.data_ptr<int32_t>(),
      cursor.data_ptr<int32_t>(), total, (int)world);
  k_route_pad<<<n_blocks(n_cap), kBlock, 0, stream>>>(
      uniq_keys.data_ptr<int64_t>(), counts.data_ptr<int32_t>(),
      m_dev.data_ptr<int32_t>(), n_cap, (int)world, (int)cap, (int)key_bits,
      send_keys.data_ptr<int64_t>(), send_cnt.data_ptr<int32_t>(),
      route_pos.data_ptr<int32_t>(), cursor.data_ptr<int32_t>(),
      error_flag.data_ptr<int32_t>());
  return {send_keys, send_cnt, route_pos};
}

torch::Tensor slots_gather_pad(torch::Tensor inverse, torch::Tensor slots) {
  int64_t nnz = inverse.numel();
  auto out = torch::empty({nnz}, slots.options());
  if (nnz == 0) return out;
  k_slots_gather_pad<<<n_blocks(nnz), kBlock, 0, current_hip_stream()>>>(
      inverse.data_ptr<int32_t>(), slots.data_ptr<int32_t>(), (int)nnz,
      out.data_ptr<int32_t>());
  return out;
}

torch::Tensor cnt_sum_pad(torch::Tensor inverse, torch::Tensor cnt,
                          int64_t m_cap) {
  int64_t nnz = inverse.numel();
  auto out = torch::empty({m_cap}, cnt.options());
  auto stream = current_hip_stream();
  zero_fill(out.data_ptr<int32_t>(), m_cap, stream);
  if (nnz)
    k_cnt_sum_pad<<<n_blocks(nnz), kBlock, 0, stream>>>(
        inverse.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), (int)nnz,
        out.data_ptr<int32_t>());
  return out;
}

torch::Tensor rows_segsum_pad(torch::Tensor grad, torch::Tensor inverse,
                              int64_t m_cap) {
  int64_t nnz = inverse.numel();
  int dim = grad.size(1);
  auto out = torch::empty({m_cap, (int64_t)dim}, grad.options());
  auto stream = current_hip_stream();
  zero_fill(out.data_ptr<float>(), m_cap * dim, stream);
  if (nnz)
    k_rows_segsum_pad<<<n_blocks(nnz * dim), kBlock, 0, stream>>>(
        grad.data_ptr<float>(), inverse.data_ptr<int32_t>(), (int)nnz, dim,
        out.data_ptr<float>());
  return out;
}

torch::Tensor gather_host_rows(torch::Tensor host_src, torch::Tensor rows) {
  TORCH_CHECK(host_src.is_pinned(), "cold slab must be pinned host memory");
  TORCH_CHECK(rows.is_cuda() && rows.scalar_type() == torch::kInt64);
  int64_t m = rows.numel();
  int dim = host_src.size(1);
  auto out = torch::empty({m, (int64_t)dim},
                          rows.options().dtype(torch::kFloat32));
  if (m == 0) return out;
  k_gather_host_rows<<<n_blocks(m * dim), kBlock, 0, current_hip_stream()>>>(
      host_src.data_ptr<float>(), rows.data_ptr<int64_t>(), m, dim,
      out.data_ptr<float>());
  return out;
}

void scatter_host_rows(torch::Tensor src, torch::Tensor rows,
                       torch::Tensor host_dst) {
  TORCH_CHECK(host_dst.is_pinned(), "cold slab must be pinned host memory");
  TORCH_CHECK(rows.is_cuda() && src.is_cuda());
  int64_t m = rows.numel();
  int dim = host_dst.size(1);
  if (m == 0) return;
  k_scatter_host_rows<<<n_blocks(m * dim), kBlock, 0, current_hip_stream()>>>(
      src.data_ptr<float>(), rows.data_ptr<int64_t>(), m, dim,
      host_dst.data_ptr<float>());
}

torch::Tensor compose_i32(torch::Tensor inv_in, torch::Tensor lut) {
  int64_t nnz = inv_in.numel();
  auto out = torch::empty({nnz}, inv_in.options());
  if (nnz == 0) return out;
  k_compose_i32<<<n_blocks(nnz), kBlock, 0, current_hip_stream()>>>(
      inv_in.data_ptr<int32_t>(), lut.data_ptr<int32_t>(), (int)nnz,
      out.data_ptr<int32_t>());
  return out;
}

torch::Tensor rows_to_padded(torch::Tensor src, torch::Tensor route_pos,
                             torch::Tensor m_dev, int64_t out_rows) {
  int n_cap = route_pos.numel();
  int dim = src.size(1);
  auto dst = torch::empty({out_rows, (int64_t)dim}, src.options());
  auto stream = current_hip_stream();
  zero_fill(dst.data_ptr<float>(), out_rows * dim, stream);
  k_rows_to_padded<<<n_blocks((int64_t)n_cap * dim), kBlock, 0, stream>>>(
      src.data_ptr<float>(), route_pos.data_ptr<int32_t>(),
      m_dev.data_ptr<int32_t>(), n_cap, dim, dst.data_ptr<float>());
  return dst;
}

// keys: None, or the received keys whose PAD_KEY elements pass C skips.
// counts_in: None, or the m counters the caller has already zeroed
// (dedup_begin) — pass C then adds into them without a fill of its own.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ht_dedup_c(
    c10::optional<torch::Tensor> keys, torch::Tensor occ_entry,
    torch::Tensor ht_compact, int64_t m,
    c10::optional<torch::Tensor> counts_in) {
  int64_t nnz = occ_entry.numel();
  auto inverse = torch::empty({nnz}, ht_compact.options());
  auto rank = torch::empty({nnz}, ht_compact.options());
  if (counts_in.has_value())
    TORCH_CHECK(counts_in->numel() == m && counts_in->is_contiguous() &&
                    counts_in->scalar_type() == torch::kInt32 &&
                    counts_in->is_cuda(),
                "ht_dedup_c: counts must be int32 [m] on GPU");
  auto counts = counts_in.has_value()
                    ? *counts_in
                    : torch::empty({m}, ht_compact.options());
  if (nnz == 0) return {inverse, counts, rank};
  auto stream = current_hip_stream();
  if (!counts_in.has_value()) zero_fill(counts.data_ptr<int32_t>(), m, stream);
  k_dedup_pass_c<<<n_blocks(nnz), kBlock, 0, stream>>>(
      opt_ptr<int64_t>(keys), occ_entry.data_ptr<int64_t>(), (int)nnz,
      ht_compact.data_ptr<int32_t>(), inverse.data_ptr<int32_t>(),
      counts.data_ptr<int32_t>(), rank.data_ptr<int32_t>());
  return {inverse, counts, rank};
}

// Exclusive prefix sum of int32 counts [m] -> int32 bounds [m + 1].
torch::Tensor csr_bounds(torch::Tensor counts) {
  CHECK_DEV(counts);
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 && counts.dim() == 1 &&
                  counts.is_contiguous(),
              "csr_bounds: counts must be contiguous int32 [m]");
  const int64_t m = counts.numel();
  if (m == 0) return torch::zeros({1}, counts.options());
  auto bounds = torch::empty({m + 1}, counts.options());
  const int64_t n_tiles = (m + kScanTile - 1) / kScanTile;
  TORCH_CHECK(n_tiles <= INT32_MAX, "csr_bounds: too many counts");
  auto tile_sums = torch::empty({n_tiles}, counts.options());
  const int grid = (int)std::min<int64_t>(n_tiles, kScanMaxBlocks);
  auto stream = current_hip_stream();
  k_tile_sums<<<grid, kBlock, 0, stream>>>(
      counts.data_ptr<int32_t>(), m, (int)n_tiles,
      tile_sums.data_ptr<int32_t>());
  k_csr_bounds<<<grid, kBlock, 0, stream>>>(
      counts.data_ptr<int32_t>(), m, (int)n_tiles,
      tile_sums.data_ptr<int32_t>(), bounds.data_ptr<int32_t>());
  return bounds;
}

torch::Tensor csr_scatter(torch::Tensor inverse, torch::Tensor rank,
                          torch::Tensor bounds, torch::Tensor error_flag) {
  int64_t nnz = inverse.numel();
  auto order = torch::empty({nnz}, inverse.options());
  if (nnz == 0) return order;
  k_csr_scatter<<<n_blocks(nnz), kBlock, 0, current_hip_stream()>>>(
      inverse.data_ptr<int32_t>(), rank.data_ptr<int32_t>(), (int)nnz,
      bounds.data_ptr<int32_t>(), order.data_ptr<int32_t>(),
      error_flag.data_ptr<int32_t>());
  return order;
}

// order over a padded stream: positions no valid occurrence lands on hold
// -1 (the segmented backward skips them). bounds has m + 1 rows.
torch::Tensor csr_scatter_pad(torch::Tensor inverse, torch::Tensor rank,
                              torch::Tensor bounds,
                              torch::Tensor error_flag) {
  int64_t nnz = inverse.numel();
  auto order = torch::empty({nnz}, inverse.options());
  if (nnz == 0) return order;
  TORCH_CHECK(rank.numel() == nnz, "csr_scatter_pad: rank size mismatch");
  TORCH_CHECK(bounds.numel() >= 1, "csr_scatter_pad: bounds is empty");
  auto stream = current_hip_stream();
  k_fill_i32<<<n_blocks(nnz), kBlock, 0, stream>>>(
      order.data_ptr<int32_t>(), nnz, -1);
  k_csr_scatter_pad<<<n_blocks(nnz), kBlock, 0, stream>>>(
      inverse.data_ptr<int32_t>(), rank.data_ptr<int32_t>(), (int)nnz,
      bounds.data_ptr<int32_t>(), (int)(bounds.numel() - 1),
      order.data_ptr<int32_t>(), error_flag.data_ptr<int32_t>());
  return order;
}

torch::Tensor csr_order(torch::Tensor inverse, torch::Tensor bounds,
                        int64_t m) {
  int64_t nnz = inverse.numel();
  auto order = torch::empty({nnz}, inverse.options());
  auto cursor = torch::zeros({m}, inverse.options());
  if (nnz == 0) return order;
  auto stream = current_hip_stream();
  k_csr_order<<<n_blocks(nnz), kBlock, 0, stream>>>(
      inverse.data_ptr<int32_t>(), (int)nnz, bounds.data_ptr<int32_t>(),
      cursor.data_ptr<int32_t>(), order.data_ptr<int32_t>());
  return order;
}

void ht_insert_bulk(torch::Tensor keys, torch::Tensor slots,
                    torch::Tensor freqs, torch::Tensor versions,
                    torch::Tensor ht_keys, torch::Tensor ht_slot,
                    torch::Tensor ht_freq, torch::Tensor ht_version,
                    torch::Tensor entry_counter, torch::Tensor error_flag) {
  int n = keys.numel();
  if (n == 0) return;
  auto stream = current_hip_stream();
  k_insert_bulk<<<n_blocks(n), kBlock, 0, stream>>>(
      keys.data_ptr<int64_t>(), slots.data_ptr<int32_t>(),
      freqs.defined() && freqs.numel() ? freqs.data_ptr<int32_t>() : nullptr,
      versions.defined() && versions.numel() ? versions.data_ptr<int64_t>()
                                             : nullptr,
      n, ht_keys.data_ptr<int64_t>(), ht_slot.data_ptr<int32_t>(),
      ht_freq.data_ptr<int32_t>(), ht_version.data_ptr<int64_t>(),
      ht_keys.numel() - 1, entry_counter.data_ptr<int32_t>(),
      error_flag.data_ptr<int32_t>());
}

std::tuple<torch::Tensor, torch::Tensor> ht_lookup(torch::Tensor keys,
                                                   torch::Tensor ht_keys,
                                                   torch::Tensor ht_slot,
                                                   bool want_entry) {
  int n = keys.numel();
  auto slots = torch::empty({n}, keys.options().dtype(torch::kInt32));
  auto entry = want_entry
                   ? torch::empty({n}, keys.options().dtype(torch::kInt64))
                   : torch::Tensor();
  if (n == 0) return {slots, entry};
  auto stream = current_hip_stream();
  k_lookup<<<n_blocks(n), kBlock, 0, stream>>>(
      keys.data_ptr<int64_t>(), n, ht_keys.data_ptr<int64_t>(),
      ht_slot.data_ptr<int32_t>(), ht_keys.numel() - 1,
      slots.data_ptr<int32_t>(),
      want_entry ? entry.data_ptr<int64_t>() : nullptr);
  return {slots, entry};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
ht_export(torch::Tensor ht_keys, torch::Tensor ht_slot, torch::Tensor ht_freq,
          torch::Tensor ht_version, int64_t n_entries) {
  auto opts_i64 = ht_keys.options();
  auto opts_i32 = ht_slot.options();
  auto out_keys = torch::empty({n_entries}, opts_i64);
  auto out_slots = torch::empty({n_entries}, opts_i32);
  auto out_freqs = torch::empty({n_entries}, opts_i32);
  auto out_versions = torch::empty({n_entries}, opts_i64);
  auto cursor = torch::zeros({1}, opts_i32);
  if (n_entries > 0) {
    auto stream = current_hip_stream();
    k_export_scan<<<n_blocks(ht_keys.numel()), kBlock, 0, stream>>>(
        ht_keys.data_ptr<int64_t>(), ht_slot.data_ptr<int32_t>(),
        ht_freq.data_ptr<int32_t>(), ht_version.data_ptr<int64_t>(),
        ht_keys.numel(), cursor.data_ptr<int32_t>(),
        out_keys.data_ptr<int64_t>(), out_slots.data_ptr<int32_t>(),
        out_freqs.data_ptr<int32_t>(), out_versions.data_ptr<int64_t>(),
        (int)n_entries);
  }
  return {out_keys, out_slots, out_freqs, out_versions};
}

torch::Tensor pooled_bwd(torch::Tensor grad_out, torch::Tensor inverse,
                         torch::Tensor offsets, torch::Tensor weights,
                         int64_t m, int64_t combiner) {
  int batch = offsets.numel() - 1;
  int dim = grad_out.size(1);
  auto grad_unique = torch::zeros(
      {m, dim}, grad_out.options().dtype(torch::kFloat32));
  if (batch == 0 || m == 0) return grad_unique;
  auto stream = current_hip_stream();
  int64_t total = (int64_t)batch * dim;
  const float* wptr =
      weights.defined() && weights.numel() ? weights.data_ptr<float>()
                                           : nullptr;
  if (grad_out.scalar_type() == torch::kBFloat16) {
    k_pooled_bwd<__hip_bfloat16><<<n_blocks(total), kBlock, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(
            grad_out.data_ptr<at::BFloat16>()),
        inverse.data_ptr<int32_t>(), offsets.data_ptr<int32_t>(), wptr, batch,
        dim, (int)combiner, grad_unique.data_ptr<float>());
  } else {
    k_pooled_bwd<float><<<n_blocks(total), kBlock, 0, stream>>>(
        grad_out.data_ptr<float>(), inverse.data_ptr<int32_t>(),
        offsets.data_ptr<int32_t>(), wptr, batch, dim, (int)combiner,
        grad_unique.data_ptr<float>());
  }
  return grad_unique;
}

// Positions of `order` per lane group in k_group_pooled_bwd_seg. From the
// {4, 8, 16, 32} sweep (profiles/PERF_LOG.md): 16 is 10 % faster on the
// zipf DLRM batch but needs 107 VGPRs (occupancy 4) and is 35 % slower on
// all-distinct keys; 8 (56 VGPRs, occupancy 8) is never slower than the
// kernel this one replaced; 32 spills.
static constexpr int kSegR = 8;

template <typename T, int LANES, int R>
static void launch_bwd_seg(const T* gp, torch::Tensor& order,
                           torch::Tensor& inverse, torch::Tensor& row_ids,
                           const float* wptr, torch::Tensor& row_coeff,
                           int64_t m, int64_t batch, int64_t n_tables,
                           int64_t dim, bool identity_rows,
                           torch::Tensor& out, hipStream_t stream) {
  int64_t nnz = order.numel();
  int64_t groups = (nnz + R - 1) / R;
  int grid = n_blocks(groups * LANES);
  if (identity_rows) {
    k_group_pooled_bwd_seg<T, LANES, R, true><<<grid, kBlock, 0, stream>>>(
        gp, order.data_ptr<int32_t>(), inverse.data_ptr<int32_t>(), nullptr,
        nullptr, nullptr, (int)nnz, (int)m, (int)batch, (int)n_tables,
        (int)dim, out.data_ptr<float>());
  } else {
    k_group_pooled_bwd_seg<T, LANES, R, false><<<grid, kBlock, 0, stream>>>(
        gp, order.data_ptr<int32_t>(), inverse.data_ptr<int32_t>(),
        row_ids.data_ptr<int32_t>(), wptr, row_coeff.data_ptr<float>(),
        (int)nnz, (int)m, (int)batch, (int)n_tables, (int)dim,
        out.data_ptr<float>());
  }
}

template <typename T, int LANES>
static void launch_bwd_seg_r(int64_t r, const T* gp, torch::Tensor& order,
                             torch::Tensor& inverse, torch::Tensor& row_ids,
                             const float* wptr, torch::Tensor& row_coeff,
                             int64_t m, int64_t batch, int64_t n_tables,
                             int64_t dim, bool identity_rows,
                             torch::Tensor& out, hipStream_t stream) {
#define SEG_CASE(RR)                                                       \
  case RR:                                                                 \
    launch_bwd_seg<T, LANES, RR>(gp, order, inverse, row_ids, wptr,        \
                                 row_coeff, m, batch, n_tables, dim,       \
                                 identity_rows, out, stream);              \
    break;
  switch (r) {
    SEG_CASE(4)
    SEG_CASE(8)
    SEG_CASE(16)
    SEG_CASE(32)
    default:
      TORCH_CHECK(false, "group_pooled_bwd_seg: r must be 4, 8, 16 or 32");
  }
#undef SEG_CASE
}

// grad_unique [m, dim] fp32 from the pooled output grad. `order` is the
// CSR occurrence order, `inverse` maps an occurrence to its unique row;
// r <= 0 selects the committed kSegR (other values exist for the sweep in
// tools/scatter_sweep.py). m may be nnz-padded (graph capture): rows
// beyond the true unique count are never referenced and stay zero.
torch::Tensor group_pooled_bwd_seg(
    torch::Tensor grad_out, torch::Tensor order, torch::Tensor inverse,
    torch::Tensor row_ids, torch::Tensor weights, torch::Tensor row_coeff,
    int64_t m, int64_t batch, int64_t n_tables, int64_t dim,
    bool identity_rows, int64_t r) {
  auto grad_unique = torch::empty(
      {m, dim}, grad_out.options().dtype(torch::kFloat32));
  if (m * dim == 0) return grad_unique;
  TORCH_CHECK(inverse.numel() == order.numel(),
              "group_pooled_bwd_seg: inverse/order size mismatch");
  TORCH_CHECK(grad_out.numel() == batch * n_tables * dim,
              "group_pooled_bwd_seg: grad_out is not [batch, n_tables*dim]");
  if (!identity_rows)
    TORCH_CHECK(row_ids.numel() == order.numel() &&
                    row_coeff.numel() == batch * n_tables,
                "group_pooled_bwd_seg: row_ids/row_coeff size mismatch");
  auto stream = current_hip_stream();
  zero_fill(grad_unique.data_ptr<float>(), m * dim, stream);
  if (order.numel() == 0) return grad_unique;
  const float* wptr =
      weights.defined() && weights.numel() ? weights.data_ptr<float>()
                                           : nullptr;
  if (wptr)
    TORCH_CHECK(weights.numel() == order.numel(),
                "group_pooled_bwd_seg: weights size mismatch");
  if (r <= 0) r = kSegR;
  if (grad_out.scalar_type() == torch::kBFloat16) {
    auto* gp = reinterpret_cast<const __hip_bfloat16*>(
        grad_out.data_ptr<at::BFloat16>());
    if (dim >= 16)
      launch_bwd_seg_r<__hip_bfloat16, 16>(
          r, gp, order, inverse, row_ids, wptr, row_coeff, m, batch,
          n_tables, dim, identity_rows, grad_unique, stream);
    else
      launch_bwd_seg_r<__hip_bfloat16, 8>(
          r, gp, order, inverse, row_ids, wptr, row_coeff, m, batch,
          n_tables, dim, identity_rows, grad_unique, stream);
  } else {
    auto* gp = grad_out.data_ptr<float>();
    if (dim >= 16)
      launch_bwd_seg_r<float, 16>(
          r, gp, order, inverse, row_ids, wptr, row_coeff, m, batch,
          n_tables, dim, identity_rows, grad_unique, stream);
    else
      launch_bwd_seg_r<float, 8>(
          r, gp, order, inverse, row_ids, wptr, row_coeff, m, batch,
          n_tables, dim, identity_rows, grad_unique, stream);
  }
  return grad_unique;
}

void register_dense(pybind11::module_& mod);      // dense_kernels.hip
void register_gru(pybind11::module_& mod);        // gru_kernels.hip
void register_attention(pybind11::module_& mod);  // attention_kernels.hip
void register_fp8(pybind11::module_& mod);        // fp8_kernels.hip
void register_ev_read(pybind11::module_& mod);    // ev_read_kernels.hip
void register_ev_apply(pybind11::module_& mod);   // ev_apply_kernels.hip
void register_loss(pybind11::module_& mod);       // loss_kernels.hip

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  register_dense(mod);
  register_gru(mod);
  register_attention(mod);
  register_fp8(mod);
  register_ev_read(mod);
  register_ev_apply(mod);
  register_loss(mod);
  mod.def("ht_lookup_insert", &ht_lookup_insert);
  mod.def("ht_dedup_a", &ht_dedup_a);
  mod.def("ht_dedup_a_pad", &ht_dedup_a_pad);
  mod.def("ht_dedup_a_matrix", &ht_dedup_a_matrix);
  mod.def("ht_dedup_b", &ht_dedup_b);
  mod.def("bump_epoch", &bump_epoch);
  mod.def("bump_epoch_only", &bump_epoch_only);
  mod.def("dedup_begin", &dedup_begin);
  mod.def("route_pad", &route_pad);
  mod.def("rows_to_padded", &rows_to_padded);
  mod.def("slots_gather_pad", &slots_gather_pad);
  mod.def("cnt_sum_pad", &cnt_sum_pad);
  mod.def("rows_segsum_pad", &rows_segsum_pad);
  mod.def("compose_i32", &compose_i32);
  mod.def("gather_host_rows", &gather_host_rows);
  mod.def("scatter_host_rows", &scatter_host_rows);
  mod.def("ht_dedup_c", &ht_dedup_c, pybind11::arg("keys"),
          pybind11::arg("occ_entry"), pybind11::arg("ht_compact"),
          pybind11::arg("m"), pybind11::arg("counts") = pybind11::none());
  mod.def("csr_bounds", &csr_bounds);
  mod.attr("CSR_SCAN_TILE") = kScanTile;
  mod.attr("CSR_SCAN_MAX_BLOCKS") = kScanMaxBlocks;
  mod.def("csr_order", &csr_order);
  mod.def("csr_scatter", &csr_scatter);
  mod.def("csr_scatter_pad", &csr_scatter_pad);
  mod.def("ht_insert_bulk", &ht_insert_bulk);
  mod.def("ht_lookup", &ht_lookup);
  mod.def("ht_export", &ht_export);
  mod.def("pooled_bwd", &pooled_bwd);
  mod.def("group_pooled_bwd_seg", &group_pooled_bwd_seg);
  mod.attr("BWD_SEG_R") = (int64_t)kSegR;
  mod.attr("EMPTY_KEY") = EMPTY_KEY;
  mod.attr("PAD_KEY") = INT64_MAX;
}
