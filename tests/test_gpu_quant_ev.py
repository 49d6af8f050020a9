"""fp8-resident embedding storage (ops/quant_backend.py) and its
dequantizing read kernels (Q8Rows in ops/hip/ev_read_kernels.hip).

Semantics under test: value(s, d) = fl32(scale[s] * decode_e4m3(q[s, d])),
which is ops.fp8.dequantize_fp8_rows, so every gather is compared exactly
(`torch.equal`) against that function on the CPU. Pooling accumulates in
fp32 in bag order, applies the combiner coefficient and rounds once; its
bound against a float64 pool is derived (tests/read_reference.py), not tuned. Bytes and scales
are asymmetric random values so a swapped byte order inside a 32-bit word
or a scale applied to the wrong row cannot cancel. 0x7F / 0xFF (the two
e4m3 NaN codes) never occur: neither the quantizer nor anything here emits
them."""
import pytest
import torch

from tests.read_reference import IDS_PER_TABLE, bags
from tests.read_reference import check_pool as _check_pool
from tests.read_reference import pool_reference as _pool_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DVD = 5           # default_values rows per table
NP_VALUE = 0.25   # no-permission fill


def _deq(q, s):
    from deeprec_amd.ops.fp8 import dequantize_fp8_rows
    return dequantize_fp8_rows(q.cpu(), s.cpu())


def _rand_rows(n, dim, gen):
    """Finite e4m3 bytes over the whole code space and scales in
    [2^-6, 2^3) (no product falls into fp32 subnormals)."""
    q = torch.randint(0, 256, (n, dim), generator=gen).to(torch.uint8)
    q[(q & 0x7F) == 0x7F] -= 1
    s = torch.exp2(torch.rand(n, generator=gen) * 9 - 6)
    return q, s


def _option(no_permission=False, evict=None, storage_type=None):
    from deeprec_amd.embedding.options import (
        CounterFilter, EmbeddingVariableOption, InitializerOption,
        StorageOption)
    opt = EmbeddingVariableOption(
        init_capacity=1024, evict_option=evict,
        init_option=InitializerOption(
            default_value_dim=DVD, default_value_no_permission=NP_VALUE))
    if no_permission:  # the fill applies only behind an admission filter
        opt.filter_option = CounterFilter(filter_freq=2)
    if storage_type is not None:
        opt.storage_option = StorageOption(storage_type=storage_type)
    return opt


def _storage(dim, **kw):
    from deeprec_amd.ops.quant_backend import QuantizedHbmStorage
    return QuantizedHbmStorage(dim, _option(**kw), device=DEV,
                               generator=torch.Generator().manual_seed(7))


def _missing_rows(st, keys, no_permission):
    """What a key without a slot reads, on the CPU."""
    dv = st.default_values.cpu()
    if no_permission:
        return torch.full((keys.numel(), st.dim), NP_VALUE)
    return dv[keys.cpu() % dv.shape[0]]


# --------------------------------------------------------------------------
# 1. decode
# --------------------------------------------------------------------------

def test_decode_matches_torch_e4m3_on_every_finite_code():
    codes = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    st = _storage(16)
    keys = torch.arange(16, dtype=torch.int64)
    st.import_quantized(keys, codes.view(16, 16), torch.ones(16))
    kd = keys.to(DEV)
    out = st.gather(kd, st.lookup(kd)).cpu().reshape(-1)
    ref = codes.view(torch.float8_e4m3fn).float()
    finite = (codes & 0x7F) != 0x7F
    assert int(finite.sum()) == 254
    assert torch.equal(out[finite], ref[finite])


# --------------------------------------------------------------------------
# 2. gather and seq gather, exact
# --------------------------------------------------------------------------

M_UNIQ = 257
NNZ = 203


def _populated(dim, no_permission):
    gen = torch.Generator().manual_seed(1000 + dim)
    q, s = _rand_rows(M_UNIQ, dim, gen)
    keys = torch.randperm(1 << 20, generator=gen)[:M_UNIQ] + (1 << 33)
    st = _storage(dim, no_permission=no_permission)
    st.import_quantized(keys, q, s)
    # query in another order, and drop every 7th slot (a known key without
    # a value row)
    perm = torch.randperm(M_UNIQ, generator=gen)
    qkeys = keys[perm].to(DEV)
    slots = st.lookup(qkeys)
    assert int((slots < 0).sum()) == 0
    slots[::7] = -1
    rows = _deq(q[perm], s[perm])
    miss = slots.cpu() < 0
    rows[miss] = _missing_rows(st, qkeys, no_permission)[miss]
    return st, qkeys, slots, rows, gen


@pytest.mark.parametrize("no_permission", [False, True],
                         ids=["default_rows", "no_permission"])
@pytest.mark.parametrize("dim", [1, 3, 4, 16, 20, 64, 130])
def test_gather_is_exact(dim, no_permission):
    st, qkeys, slots, rows, _ = _populated(dim, no_permission)
    out = st.gather(qkeys, slots)
    assert out.dtype == torch.float32
    assert torch.equal(out.cpu(), rows)
    out16 = st.gather(qkeys, slots, torch.bfloat16)
    assert torch.equal(out16.cpu(), rows.to(torch.bfloat16))


@pytest.mark.parametrize("no_permission", [False, True],
                         ids=["default_rows", "no_permission"])
@pytest.mark.parametrize("dim", [1, 3, 4, 16, 20, 64, 130])
def test_seq_gather_pad_is_exact(dim, no_permission):
    st, qkeys, slots, rows, gen = _populated(dim, no_permission)
    inverse = torch.randint(0, M_UNIQ, (NNZ,), generator=gen,
                            dtype=torch.int32)
    inverse[::5] = -1
    inverse[3::11] = M_UNIQ              # first index past n_uniq
    inverse[7] = 2 ** 31 - 1
    inverse[8] = -(2 ** 31)
    valid = (inverse >= 0) & (inverse < M_UNIQ)
    ref = torch.zeros(NNZ, dim)
    ref[valid] = rows[inverse[valid].long()]
    out = st.seq_gather_pad(qkeys, slots, inverse.to(DEV))
    assert torch.equal(out.cpu(), ref)
    out16 = st.seq_gather_pad(qkeys, slots, inverse.to(DEV), torch.bfloat16)
    assert torch.equal(out16.cpu(), ref.to(torch.bfloat16))


# --------------------------------------------------------------------------
# 3. pooled and group pooled
# --------------------------------------------------------------------------
#
# The bound, derived in tests/read_reference.py:
#     |out - ref| <= (L + 2) * 2^-24 * coeff * sum_j |w_j v_j|,
# plus 2^-8 * |ref| for a bf16 output.

BATCH, N_TABLES = 7, 3
COMBINERS = ["sum", "mean", "sqrtn"]


def _bags(gen, weighted, n_rows):
    return bags(gen, weighted, n_rows, DEV)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("dim", [3, 4, 16, 20])
def test_pooled_lookup_bound(dim, combiner, weighted):
    gen = torch.Generator().manual_seed(31 * dim + weighted)
    q, s = _rand_rows(IDS_PER_TABLE, dim, gen)
    st = _storage(dim)
    st.import_quantized(torch.arange(IDS_PER_TABLE), q, s)
    table = torch.cat([_deq(q, s), torch.zeros(5, dim)])
    dv = st.default_values.cpu()
    for k in range(IDS_PER_TABLE, IDS_PER_TABLE + 5):
        table[k] = dv[k % DVD]
    sp, ids, offsets, w = _bags(gen, weighted, BATCH)
    uniq, inverse = torch.unique(sp.values, return_inverse=True)
    slots = st.lookup(uniq)
    assert int((slots < 0).sum()) > 0     # missing keys are in play
    ref, mag, lens = _pool_reference(lambda i: table[i], ids, offsets, w,
                                     combiner)
    for dtype in (torch.float32, torch.bfloat16):
        out = st.pooled_lookup(uniq, slots, inverse, sp.offsets,
                               sp.row_ids(), combiner, sp.weights, dtype)
        assert out.dtype == dtype and tuple(out.shape) == (BATCH, dim)
        _check_pool(out, ref, mag, lens, f"pooled {combiner} {dtype}")


def _fp8_collection(dim, name="q8", n_tables=N_TABLES, combiners=None):
    from deeprec_amd.embedding.collection import EmbeddingCollection
    from deeprec_amd.embedding.options import StorageType
    return EmbeddingCollection(
        name, [f"t{i}" for i in range(n_tables)], dim,
        ev_option=_option(storage_type=StorageType.HBM_FP8),
        combiners=combiners or COMBINERS, device=DEV,
        generator=torch.Generator().manual_seed(7))


def _fill_collection(coll, gen, ids_per_table=IDS_PER_TABLE):
    """Random rows for ids 0..ids_per_table-1 of every table; returns the
    dequantized rows [n_tables, ids_per_table, dim]."""
    deq = []
    for t in range(coll.n_tables):
        q, s = _rand_rows(ids_per_table, coll.dim, gen)
        coll.storage.import_quantized(
            coll.composite(t, torch.arange(ids_per_table)), q, s)
        deq.append(_deq(q, s))
    return torch.stack(deq)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dim", [3, 4, 16, 20])
def test_group_pooled_lookup_bound(dim, weighted):
    gen = torch.Generator().manual_seed(77 * dim + weighted)
    coll = _fp8_collection(dim)
    assert coll.trainable is False
    deq = _fill_collection(coll, gen)
    dv = coll.storage.default_values.cpu()     # [n_tables * DVD, dim]
    sps, refs = [], []
    for t in range(N_TABLES):
        table = torch.cat([deq[t], torch.zeros(5, dim)])
        for k in range(IDS_PER_TABLE, IDS_PER_TABLE + 5):
            table[k] = dv[t * DVD + k % DVD]
        sp, ids, offsets, w = _bags(gen, weighted, BATCH)
        sps.append(sp)
        refs.append(_pool_reference(lambda i, tb=table: tb[i], ids, offsets,
                                    w, COMBINERS[t]))
    for dtype in (torch.float32, torch.bfloat16):
        # train=True on an inference-only collection serves
        out = coll.lookup(sps, out_dtype=dtype, train=True)
        assert out.dtype == dtype
        assert tuple(out.shape) == (BATCH, N_TABLES * dim)
        for t, (ref, mag, lens) in enumerate(refs):
            _check_pool(out[:, t * dim:(t + 1) * dim], ref, mag, lens,
                        f"group {COMBINERS[t]} {dtype}")


def _fp32_twin(coll, name="twin"):
    """A plain fp32 collection holding the dequantized rows of `coll`, with
    the same default rows."""
    from deeprec_amd.embedding.collection import EmbeddingCollection
    twin = EmbeddingCollection(
        name, coll.table_names, coll.dim, ev_option=_option(),
        combiners=coll.combiners, device=DEV,
        generator=torch.Generator().manual_seed(7))
    assert torch.equal(twin.storage.default_values,
                       coll.storage.default_values)
    twin.restore(*coll.export())
    return twin


@pytest.mark.parametrize("dim", [4, 16, 20, 3])
def test_single_id_bags_bit_equal_fp32_kernel(dim):
    """lookup_matrix shape, mean: both kernels compute fl32(s * q), then
    0 + 1 * v, then * 1 — the outputs must be the same bits."""
    gen = torch.Generator().manual_seed(5 * dim)
    coll = _fp8_collection(dim, combiners=["mean"] * N_TABLES)
    _fill_collection(coll, gen)
    twin = _fp32_twin(coll)
    ids = torch.randint(0, IDS_PER_TABLE + 5, (BATCH * 37, N_TABLES),
                        generator=gen).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        out = coll.lookup_matrix(ids, out_dtype=dtype, train=False)
        ref = twin.lookup_matrix(ids, out_dtype=dtype, train=False)
        assert torch.equal(out, ref)


# --------------------------------------------------------------------------
# 4. grid stride: thread counts past the 65535 x 256 launch cap
# --------------------------------------------------------------------------

def test_seq_gather_pad_grid_strides_past_the_cap():
    dim, rows, nnz = 16, 1024, 4_194_561
    assert nnz * (dim // 4) > 65535 * 256
    gen = torch.Generator().manual_seed(4)
    q, s = _rand_rows(rows, dim, gen)
    st = _storage(dim)
    keys = torch.arange(rows)
    st.import_quantized(keys, q, s)
    kd = keys.to(DEV)
    slots = st.lookup(kd)
    inverse = torch.randint(0, rows, (nnz,), device=DEV, dtype=torch.int32)
    inverse[-1] = rows - 1                 # the very last thread's row
    out = st.seq_gather_pad(kd, slots, inverse, torch.bfloat16)
    table = _deq(q, s).to(torch.bfloat16).to(DEV)   # row u belongs to key u
    assert torch.equal(out, table[inverse.long()])


def test_group_pooled_grid_strides_past_the_cap():
    dim, n_tables, batch, per = 16, 26, 161_321, 40
    assert batch * n_tables * (dim // 4) > 65535 * 256
    gen = torch.Generator().manual_seed(5)
    coll = _fp8_collection(dim, n_tables=n_tables,
                           combiners=["mean"] * n_tables)
    deq = _fill_collection(coll, gen, per).to(DEV)      # [26, 40, 16]
    ids = torch.randint(0, per, (batch, n_tables), device=DEV)
    out = coll.lookup_matrix(ids, train=False)
    ref = deq[torch.arange(n_tables, device=DEV)[None, :], ids]
    assert torch.equal(out, ref.reshape(batch, n_tables * dim))


# --------------------------------------------------------------------------
# 5. import
# --------------------------------------------------------------------------

def _fp32_rows(n, dim, gen):
    """Rows spanning e4m3's normal and subnormal range relative to the row
    maximum, with an all-zero row."""
    v = torch.randn(n, dim, generator=gen)
    v *= torch.exp2(torch.randint(-12, 1, (n, dim), generator=gen).float())
    v[:, 0] = torch.randn(n, generator=gen) * 3      # a dominant element
    v[n // 2] = 0.0
    return v


@pytest.mark.parametrize("dim", [3, 16])
def test_import_quantizes_within_half_an_e4m3_ulp(dim, monkeypatch):
    from deeprec_amd.ops import quant_backend
    # several chunks, the last one ragged
    monkeypatch.setattr(quant_backend, "_CHUNK_ROWS", 100)
    gen = torch.Generator().manual_seed(dim)
    n = 257
    v = _fp32_rows(n, dim, gen)
    keys = torch.arange(n) * 3 + 11               # sorted, as export sorts
    st = _storage(dim)
    st.import_(keys, v, torch.arange(n), torch.arange(n) + 1)
    k, q, s, freqs, versions = st.export_quantized()
    assert torch.equal(k.cpu(), keys)
    assert torch.equal(freqs.cpu(), torch.arange(n))
    assert torch.equal(versions.cpu(), torch.arange(n) + 1)
    amax = v.abs().amax(dim=1)
    want_s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.equal(s.cpu(), want_s)
    assert int(((q.cpu() & 0x7F) == 0x7F).sum()) == 0   # finite codes only
    deq = _deq(q, s)
    bound = torch.maximum(v.abs() * 2.0 ** -4,
                          want_s[:, None] * 2.0 ** -10) * (1 + 2.0 ** -10)
    err = (deq - v).abs()
    print("import: max err/bound =",
          float((err / bound.clamp(min=1e-30)).max()))
    assert bool((err <= bound).all())
    # zero row: zero bytes, unit scale
    assert int(q[n // 2].cpu().sum()) == 0 and float(s[n // 2]) == 1.0
    # export() hands the Saver the dequantized rows
    ek, ev, _, _ = st.export()
    assert torch.equal(ek.cpu(), keys) and torch.equal(ev.cpu(), deq)


def test_import_quantized_round_trips_bits():
    gen = torch.Generator().manual_seed(9)
    n, dim = 300, 20
    q, s = _rand_rows(n, dim, gen)
    keys = torch.arange(n) * 5 + 2
    st = _storage(dim)
    st.import_quantized(keys, q, s, torch.arange(n), torch.arange(n))
    k, q2, s2, _, _ = st.export_quantized()
    assert torch.equal(k.cpu(), keys)
    assert torch.equal(q2.cpu(), q) and torch.equal(s2.cpu(), s)
    with pytest.raises(ValueError, match="import_quantized"):
        st.import_quantized(keys, q.float(), s)


# --------------------------------------------------------------------------
# 6. storage life cycle
# --------------------------------------------------------------------------

def test_growth_keeps_bytes_and_scales():
    gen = torch.Generator().manual_seed(6)
    dim = 16
    st = _storage(dim)
    first = st.max_slots
    q, s = _rand_rows(first + 500, dim, gen)
    keys = torch.arange(first + 500) * 2
    st.import_quantized(keys[:600], q[:600], s[:600])
    assert st.max_slots == first
    st.import_quantized(keys[600:], q[600:], s[600:])
    assert st.max_slots > first
    _, q2, s2, _, _ = st.export_quantized()
    assert torch.equal(q2.cpu(), q) and torch.equal(s2.cpu(), s)
    mu = st.memory_usage()
    assert st.values.dtype == torch.uint8 and st.scales.dtype == torch.float32
    assert mu["values_bytes"] == st.max_slots * dim
    assert mu["scale_bytes"] == st.max_slots * 4
    assert mu["slab_bytes"] == 0
    assert mu["total_bytes"] == (mu["table_bytes"] + mu["values_bytes"]
                                 + mu["scale_bytes"])
    # delta update: an existing key keeps its slot, the row is replaced
    kd = keys[5:6].to(DEV)
    slot = int(st.lookup(kd))
    st.import_quantized(keys[5:6], q[9:10], s[9:10])
    assert int(st.lookup(kd)) == slot
    assert torch.equal(st.values[slot].cpu(), q[9])
    assert float(st.scales[slot]) == float(s[9])


def test_shrink_keeps_surviving_rows():
    from deeprec_amd.embedding.options import GlobalStepEvict, L2WeightEvict
    gen = torch.Generator().manual_seed(8)
    n, dim = 200, 16
    q, s = _rand_rows(n, dim, gen)
    keys = torch.arange(n) + 1000
    versions = torch.where(torch.arange(n) % 3 == 0,
                           torch.tensor(100), torch.tensor(0))
    st = _storage(dim, evict=GlobalStepEvict(steps_to_live=5))
    st.import_quantized(keys, q, s, torch.ones(n, dtype=torch.int64),
                        versions)
    keep = versions >= 95
    assert st.shrink(100) == int((~keep).sum())
    k, q2, s2, _, v2 = st.export_quantized()
    assert torch.equal(k.cpu(), keys[keep])
    assert torch.equal(q2.cpu(), q[keep]) and torch.equal(s2.cpu(), s[keep])
    assert torch.equal(v2.cpu(), versions[keep])

    # L2 eviction measures the DEQUANTIZED rows
    # (threshold midway between two rows' norms, so the device norm's last
    # bit cannot move a row across it)
    norms = _deq(q, s).norm(dim=1)
    srt = norms.sort().values
    thr = float((srt[n // 2 - 1] + srt[n // 2]) / 2)
    st = _storage(dim, evict=L2WeightEvict(l2_weight_threshold=thr))
    st.import_quantized(keys, q, s)
    keep = norms >= thr
    assert st.shrink(0) == int((~keep).sum())
    k, q2, s2, _, _ = st.export_quantized()
    assert torch.equal(k.cpu(), keys[keep])
    assert torch.equal(q2.cpu(), q[keep]) and torch.equal(s2.cpu(), s[keep])


def test_training_entry_points_raise():
    from deeprec_amd.ops.hip_backend import sparse_apply
    st = _storage(16)
    keys = torch.arange(4, device=DEV)
    calls = [
        lambda: st.get_slab("adam_m", 16, 0.0),
        lambda: st.enable_graph_mode(1024, 1024),
        lambda: st.dedup_lookup(keys, 0),
        lambda: st.dedup_lookup_capture(keys),
        lambda: st.dedup_only_capture(keys),
        lambda: st.dedup_lookup_capture_owner(keys, keys.int()),
        lambda: st.lookup_or_create(keys, None, 0, train=True),
        lambda: sparse_apply("sgd", st, keys.int(),
                             torch.zeros(4, 16, device=DEV), {"lr": 0.1}),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="inference-only"):
            call()
    # the find itself works and admits nothing
    assert torch.equal(st.lookup_or_create(keys, None, 0, train=False).cpu(),
                       torch.full((4,), -1, dtype=torch.int32))
    assert st.total_count() == 0


def test_ev_with_hbm_fp8_storage_type_serves():
    from deeprec_amd.embedding import (EmbeddingVariable, RaggedIds,
                                       embedding_lookup,
                                       embedding_lookup_sparse)
    from deeprec_amd.embedding.options import StorageType
    from deeprec_amd.ops.quant_backend import QuantizedHbmStorage
    gen = torch.Generator().manual_seed(12)
    ev = EmbeddingVariable("fp8ev", 16, device=DEV,
                           ev_option=_option(
                               storage_type=StorageType.HBM_FP8))
    assert isinstance(ev.storage, QuantizedHbmStorage)
    assert ev.trainable is False and not ev._anchor.requires_grad
    v = torch.randn(50, 16, generator=gen)
    ev.restore(torch.arange(50), v)
    _, q, s, _, _ = ev.storage.export_quantized()
    deq = _deq(q, s)
    ids = torch.randint(0, 50, (6, 9), generator=gen)
    # an EV passes train through to the storage, which refuses it
    with pytest.raises(RuntimeError, match="inference-only"):
        embedding_lookup(ev, ids.to(DEV), train=True)
    out = embedding_lookup(ev, ids.to(DEV), train=False)
    assert torch.equal(out.cpu(), deq[ids])
    # padded static-shape path: zero rows at the pad id
    ids[:, -2:] = -1
    out = embedding_lookup(ev, ids.to(DEV), pad_id=-1, train=False)
    ref = deq[ids.clamp(min=0)]
    ref[ids < 0] = 0.0
    assert torch.equal(out.cpu(), ref)
    # two-id bags: the sum is one addition, exact in any order
    sp = RaggedIds(torch.arange(4, device=DEV),
                   torch.tensor([0, 2, 2, 4], dtype=torch.int32, device=DEV))
    out = embedding_lookup_sparse(ev, sp, combiner="sum", train=False)
    ref = torch.stack([deq[0] + deq[1], torch.zeros(16), deq[2] + deq[3]])
    assert torch.equal(out.cpu(), ref)


# --------------------------------------------------------------------------
# 7. converter
# --------------------------------------------------------------------------

def test_converter_swaps_a_trained_collection_in_place():
    from deeprec_amd.embedding.collection import EmbeddingCollection
    from deeprec_amd.ops.fp8 import quantize_embeddings_fp8
    from deeprec_amd.ops.quant_backend import QuantizedHbmStorage
    from deeprec_amd.optimizers import AdamOptimizer
    gen = torch.Generator().manual_seed(21)
    dim = 16
    coll = EmbeddingCollection("conv", ["a", "b", "c"], dim,
                               ev_option=_option(),
                               combiners=["mean"] * 3, device=DEV)
    opt = AdamOptimizer(embedding_variables=[coll], learning_rate=0.05)
    for _ in range(3):                       # ~2k keys, Adam slabs exist
        ids = torch.randint(0, 700, (512, 3), generator=gen).to(DEV)
        out = coll.lookup_matrix(ids, train=True)
        opt.zero_grad()
        (out * out).sum().backward()
        opt.step()
    assert coll.storage.slabs and coll.size() > 1500
    old = coll.storage
    keys, values, freqs, versions = coll.export()
    before = old.memory_usage()

    assert quantize_embeddings_fp8(coll) == 1
    st = coll.storage
    assert type(st) is QuantizedHbmStorage
    assert st.values.dtype == torch.uint8 and st.slabs == {}
    assert old.values is None and old.slabs == {}
    assert st.ht_keys is old.ht_keys          # the table is taken over
    assert coll.trainable is False
    after = st.memory_usage()
    assert after["values_bytes"] * 4 == before["values_bytes"]
    assert after["slab_bytes"] == 0
    assert quantize_embeddings_fp8(coll) == 0  # already converted

    # same keys and metadata; rows within the e4m3 half-ulp
    k2, q, s, f2, v2 = st.export_quantized()
    assert torch.equal(k2, keys) and torch.equal(f2, freqs)
    assert torch.equal(v2, versions)
    # rows quantize independently: the chunked conversion gives the bytes
    # the row quantizer gives on the exported fp32 rows
    q_ref, s_ref = st.ext.quant_rows_e4m3(values.contiguous())
    assert torch.equal(q, q_ref) and torch.equal(s, s_ref)

    twin = EmbeddingCollection("conv_twin", ["a", "b", "c"], dim,
                               ev_option=_option(), combiners=["mean"] * 3,
                               device=DEV)
    twin.storage.default_values.copy_(st.default_values)
    twin.restore(*coll.export())
    ids = torch.randint(0, 800, (300, 3), generator=gen).to(DEV)
    n_entries = st.total_count()
    for dtype in (torch.float32, torch.bfloat16):
        # train=True serves: no admission, no autograd graph
        out = coll.lookup_matrix(ids, out_dtype=dtype, train=True)
        assert not out.requires_grad
        assert torch.equal(out, twin.lookup_matrix(ids, out_dtype=dtype,
                                                   train=False))
    assert st.total_count() == n_entries


# --------------------------------------------------------------------------
# 8. predictor
# --------------------------------------------------------------------------

def _tiny_dlrm(prefix):
    from deeprec_amd.models.dlrm import DLRM
    return DLRM(embedding_dim=16, mlp_bot=(32, 16), mlp_top=(32,),
                bf16=False, device=DEV, ev_option=_option(), num_sparse=3,
                name_prefix=prefix)


def test_predictor_serves_fp8_embeddings_and_requantizes_deltas(tmp_path):
    from deeprec_amd.checkpoint.saver import Saver
    from deeprec_amd.embedding.variable import GLOBAL_STEP
    from deeprec_amd.optimizers import AdamOptimizer
    from deeprec_amd.ops.quant_backend import QuantizedHbmStorage
    from deeprec_amd.serving.predictor import Predictor
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(33)
    m = _tiny_dlrm("pm")
    opt = AdamOptimizer(params=m.parameters(),
                        embedding_variables=m.embedding_variables(),
                        learning_rate=0.05)
    saver = Saver(module=m, embedding_variables=m.embedding_variables(),
                  optimizer=opt)

    def train(dense, ids):
        loss = m.loss_fn(m(dense, ids), torch.ones(ids.shape[0], device=DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()

    for _ in range(2):
        train(torch.randn(64, 13, generator=gen).to(DEV),
              torch.randint(0, 50, (64, 3), generator=gen).to(DEV))
    saver.save(str(tmp_path), GLOBAL_STEP.value)

    def serving_model(prefix):
        ms = _tiny_dlrm(prefix)
        ms.collection.name = m.collection.name
        return ms

    p8 = Predictor(serving_model("p8"), str(tmp_path), num_sessions=1,
                   fp8_embeddings=True)
    st8 = p8.model.collection.storage
    assert type(st8) is QuantizedHbmStorage and st8.slabs == {}
    assert st8.size() == m.collection.size()
    plain = Predictor(serving_model("pp"), str(tmp_path), num_sessions=1)
    assert plain.model.collection.storage.slabs      # Adam slabs restored
    plain.model.collection.restore(*p8.model.collection.export())

    dense = torch.randn(40, 13, generator=gen).to(DEV)
    ids = torch.randint(0, 50, (40, 3), generator=gen).to(DEV)
    # keep to keys the checkpoint holds: the two models' default rows differ
    present = (st8.lookup(p8.model.collection.matrix_inputs(ids)[0]) >= 0
               ).reshape(3, -1).all(0)
    dense, ids = dense[present], ids[present]
    assert ids.shape[0] > 10
    a, b = plain.predict(dense, ids), plain.predict(dense, ids)
    if torch.equal(a, b):
        assert torch.equal(p8.predict(dense, ids), a)
    else:
        # the dense forward is not bit-stable run to run on this stack:
        # compare where the feature ends, at the lookup output
        assert torch.equal(
            p8.model.collection.lookup_matrix(ids, train=False),
            plain.model.collection.lookup_matrix(ids, train=False))

    # delta: one sample whose three ids are two existing keys and a new one
    k0, q0, s0, _, _ = st8.export_quantized()
    d_ids = torch.tensor([[int(ids[0, 0]), int(ids[0, 1]), 999]] * 8,
                         device=DEV)
    touched = torch.unique(m.collection.matrix_inputs(d_ids)[0])
    assert touched.numel() == 3
    assert int((st8.lookup(touched) >= 0).sum()) == 2
    train(torch.randn(8, 13, generator=gen).to(DEV), d_ids)
    saver.incremental_save(str(tmp_path), GLOBAL_STEP.value)
    assert p8.poll_updates() == 1
    assert st8 is p8.model.collection.storage and st8.slabs == {}

    k1, q1, s1, _, _ = st8.export_quantized()
    assert k1.numel() == k0.numel() + 1
    is_touched = torch.isin(k1, touched)
    assert int(is_touched.sum()) == 3
    # untouched rows: bytes and scales unchanged
    assert torch.equal(k1[~is_touched], k0[~torch.isin(k0, touched)])
    assert torch.equal(q1[~is_touched], q0[~torch.isin(k0, touched)])
    assert torch.equal(s1[~is_touched], s0[~torch.isin(k0, touched)])
    # touched rows: the trainer's current fp32 rows within the import bound
    slots = m.collection.storage.lookup(k1[is_touched])
    v = m.collection.storage.gather(k1[is_touched], slots).cpu()
    assert float((v[:2] - _deq(q0[torch.isin(k0, touched)],
                               s0[torch.isin(k0, touched)])).abs().max()) > 0
    sc = v.abs().amax(dim=1) / 448.0
    bound = torch.maximum(v.abs() * 2.0 ** -4,
                          sc[:, None] * 2.0 ** -10) * (1 + 2.0 ** -10)
    err = (_deq(q1[is_touched], s1[is_touched]) - v).abs()
    assert bool((err <= bound).all())
