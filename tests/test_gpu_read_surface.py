"""The embedding read surface (ops/hip/ev_read_kernels.hip) on its fp32 and
pre-gathered ("direct") row sources: the missing-key paths of the gather
and pooled kernels against CPU references, and the shared kernel body
pinned bit for bit across row sources and across the single-table and
group kernels. The fp8 source has the same cases in test_gpu_quant_ev.py.

Gathers copy fp32 values (one rounding for bf16), so they are compared
exactly. Pooled outputs are held to the bound derived in
tests/read_reference.py, not a tuned one."""
import pytest
import torch

from tests.read_reference import (IDS_PER_TABLE, bags, check_pool,
                                  pool_reference)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DVD = 5           # default_values rows per table
NP_VALUE = 0.25   # no-permission fill
M_UNIQ = 257
BATCH, N_TABLES = 7, 3
COMBINERS = ["sum", "mean", "sqrtn"]


def _option(no_permission=False):
    from deeprec_amd.embedding.options import (
        CounterFilter, EmbeddingVariableOption, InitializerOption)
    opt = EmbeddingVariableOption(
        init_capacity=1024,
        init_option=InitializerOption(
            default_value_dim=DVD, default_value_no_permission=NP_VALUE))
    if no_permission:  # the fill applies only behind an admission filter
        opt.filter_option = CounterFilter(filter_freq=2)
    return opt


def _storage(dim, **kw):
    from deeprec_amd.ops.hip_backend import HbmStorage
    return HbmStorage(dim, _option(**kw), device=DEV,
                      generator=torch.Generator().manual_seed(7))


def _rand_rows(n, dim, gen):
    """Asymmetric rows: no two columns or rows can be swapped unnoticed."""
    return torch.randn(n, dim, generator=gen) * 2


# --------------------------------------------------------------------------
# 1. gather, exact
# --------------------------------------------------------------------------

@pytest.mark.parametrize("no_permission", [False, True],
                         ids=["default_rows", "no_permission"])
@pytest.mark.parametrize("dim", [1, 3, 4, 16, 20])
def test_gather_is_exact(dim, no_permission):
    gen = torch.Generator().manual_seed(1000 + dim)
    v = _rand_rows(M_UNIQ, dim, gen)
    keys = torch.randperm(1 << 20, generator=gen)[:M_UNIQ] + (1 << 33)
    st = _storage(dim, no_permission=no_permission)
    st.import_(keys, v)
    # query in another order, and drop every 7th slot (a known key without
    # a value row)
    perm = torch.randperm(M_UNIQ, generator=gen)
    qkeys = keys[perm].to(DEV)
    slots = st.lookup(qkeys)
    assert int((slots < 0).sum()) == 0
    slots[::7] = -1
    rows = v[perm].clone()
    miss = slots.cpu() < 0
    dv = st.default_values.cpu()
    assert dv.shape[0] == DVD
    rows[miss] = (torch.full((M_UNIQ, dim), NP_VALUE) if no_permission
                  else dv[keys[perm] % DVD])[miss]
    out = st.gather(qkeys, slots)
    assert out.dtype == torch.float32
    assert torch.equal(out.cpu(), rows)
    out16 = st.gather(qkeys, slots, torch.bfloat16)
    assert torch.equal(out16.cpu(), rows.to(torch.bfloat16))


# --------------------------------------------------------------------------
# 2. single-table pooled, bounded
# --------------------------------------------------------------------------

def _single_table(dim, gen):
    """A storage holding ids 0..39, and the CPU table of what every id
    0..44 reads (40..44 are missing: their default rows)."""
    v = _rand_rows(IDS_PER_TABLE, dim, gen)
    st = _storage(dim)
    st.import_(torch.arange(IDS_PER_TABLE), v)
    table = torch.cat([v, torch.zeros(5, dim)])
    dv = st.default_values.cpu()
    for k in range(IDS_PER_TABLE, IDS_PER_TABLE + 5):
        table[k] = dv[k % DVD]
    return st, table


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("dim", [3, 4, 16, 20])
def test_pooled_lookup_bound(dim, combiner, weighted):
    gen = torch.Generator().manual_seed(31 * dim + weighted)
    st, table = _single_table(dim, gen)
    sp, ids, offsets, w = bags(gen, weighted, BATCH, DEV)
    assert int(offsets[1]) == 0 and int(offsets[2]) == 5
    uniq, inverse = torch.unique(sp.values, return_inverse=True)
    slots = st.lookup(uniq)
    assert int((slots < 0).sum()) > 0     # missing keys are in play
    ref, mag, lens = pool_reference(lambda i: table[i], ids, offsets, w,
                                    combiner)
    for dtype in (torch.float32, torch.bfloat16):
        out = st.pooled_lookup(uniq, slots, inverse, sp.offsets,
                               sp.row_ids(), combiner, sp.weights, dtype)
        assert out.dtype == dtype and tuple(out.shape) == (BATCH, dim)
        check_pool(out, ref, mag, lens, f"pooled {combiner} {dtype}")


@pytest.mark.parametrize("combiner", ["mean", "sqrtn"])
@pytest.mark.parametrize("dim", [3, 4])
def test_pooled_coefficient_is_applied_once_after_the_sum(dim, combiner):
    """Small-integer rows and weights: every product and partial sum is
    exact in fp32, so the only roundings are the coefficient (a correctly
    rounded sqrt and divide) and the one multiply after the sum, which
    fp32 on the CPU reproduces bit for bit. A coefficient folded into each
    product rounds per term and lands on other bits. Stored keys only: the
    default rows are not integers."""
    gen = torch.Generator().manual_seed(17 * dim)
    v = torch.randint(-8, 9, (IDS_PER_TABLE, dim), generator=gen).float()
    st = _storage(dim)
    st.import_(torch.arange(IDS_PER_TABLE), v)
    sp, ids, offsets, _ = bags(gen, False, BATCH, DEV)
    ids = ids % IDS_PER_TABLE
    w = torch.randint(1, 4, (ids.numel(),), generator=gen).float()
    ref = torch.zeros(BATCH, dim)
    for r in range(BATCH):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        if hi == lo:
            continue
        acc = (w[lo:hi, None] * v[ids[lo:hi]]).sum(0)
        wsum = w[lo:hi].sum() if combiner == "mean" \
            else (w[lo:hi] * w[lo:hi]).sum().sqrt()
        ref[r] = acc * (torch.tensor(1.0) / wsum)
    assert ref.dtype == torch.float32
    uniq, inverse = torch.unique(ids.to(DEV), return_inverse=True)
    slots = st.lookup(uniq)
    assert int((slots < 0).sum()) == 0
    for dtype in (torch.float32, torch.bfloat16):
        out = st.pooled_lookup(uniq, slots, inverse, sp.offsets,
                               sp.row_ids(), combiner, w.to(DEV), dtype)
        assert torch.equal(out.cpu(), ref.to(dtype))


# --------------------------------------------------------------------------
# 3. group pooled, bounded; 4. direct rows equal slot rows
# --------------------------------------------------------------------------

def _group_case(dim, weighted):
    """A 3-table collection (one combiner each) holding ids 0..39 of every
    table, one set of bags per table, and per table the fp64 reference
    with a missing key reading ITS table's block of default_values."""
    from deeprec_amd.embedding.collection import EmbeddingCollection
    gen = torch.Generator().manual_seed(77 * dim + weighted)
    coll = EmbeddingCollection(
        "rs", [f"t{i}" for i in range(N_TABLES)], dim, ev_option=_option(),
        combiners=COMBINERS, device=DEV,
        generator=torch.Generator().manual_seed(7))
    dv = coll.storage.default_values.cpu()     # [N_TABLES * DVD, dim]
    assert dv.shape[0] == N_TABLES * DVD
    # the blocks differ, so a default row of the wrong table is caught
    assert not torch.equal(dv[:DVD], dv[DVD:2 * DVD])
    sps, refs = [], []
    for t in range(N_TABLES):
        v = _rand_rows(IDS_PER_TABLE, dim, gen)
        coll.restore_table(t, torch.arange(IDS_PER_TABLE), v)
        table = torch.cat([v, torch.zeros(5, dim)])
        for k in range(IDS_PER_TABLE, IDS_PER_TABLE + 5):
            table[k] = dv[t * DVD + k % DVD]
        sp, ids, offsets, w = bags(gen, weighted, BATCH, DEV)
        sps.append(sp)
        refs.append(pool_reference(lambda i, tb=table: tb[i], ids, offsets,
                                   w, COMBINERS[t]))
    return coll, sps, refs


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dim", [3, 4, 16, 20])
def test_group_pooled_lookup_bound(dim, weighted):
    coll, sps, refs = _group_case(dim, weighted)
    for dtype in (torch.float32, torch.bfloat16):
        out = coll.lookup(sps, out_dtype=dtype, train=False)
        assert out.dtype == dtype
        assert tuple(out.shape) == (BATCH, N_TABLES * dim)
        for t, (ref, mag, lens) in enumerate(refs):
            check_pool(out[:, t * dim:(t + 1) * dim], ref, mag, lens,
                       f"group {COMBINERS[t]} {dtype}")
    assert coll.size() == N_TABLES * IDS_PER_TABLE   # nothing was admitted


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dim", [3, 4, 16, 20])
def test_direct_rows_equal_slot_rows_bit_for_bit(dim, weighted):
    """DirectRows and F32Rows feed the same fp32 values through the same
    bag function: the outputs must be the same bits."""
    from deeprec_amd.ops.common import KEY_BITS
    coll, sps, _ = _group_case(dim, weighted)
    st = coll.storage
    batch, values_cat, offsets_cat, _, weights_cat = coll._concat_inputs(sps)
    d = coll._dedup_and_probe(values_cat, False)
    assert int((d.slots < 0).sum()) > 0   # missing keys are in play
    rows = st.gather(d.uniq, d.slots)
    # storage.gather() hashes the whole composite key into default_values,
    # the group kernel the raw id into the table's block: give the missing
    # keys' pre-gathered rows the group's default rows
    miss = d.slots < 0
    tid, raw = coll.decompose(d.uniq[miss])
    rows[miss] = st.default_values[tid * DVD + raw % DVD]
    weights = weights_cat if weights_cat is not None else torch.Tensor()
    for dtype in (torch.float32, torch.bfloat16):
        direct = st.ext.group_pooled_fwd_direct(
            rows, d.uniq, d.inverse, offsets_cat, weights,
            coll._combiner_ids, batch, N_TABLES, dtype)
        slotted = st.ext.group_pooled_fwd(
            st.values, st.default_values, d.uniq, d.slots, d.inverse,
            offsets_cat, weights, coll._combiner_ids, batch, N_TABLES,
            KEY_BITS, st._no_permission_value(), st._use_no_permission(),
            dtype)
        assert direct.dtype == dtype
        assert torch.equal(direct, slotted)
        assert torch.equal(slotted,
                           coll.lookup(sps, out_dtype=dtype, train=False))


# --------------------------------------------------------------------------
# 5. the single-table kernel equals a one-table group launch
# --------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("dim", [3, 4, 16, 20])
def test_single_table_equals_one_table_group(dim, combiner, weighted):
    from deeprec_amd.ops.common import COMBINER_ID
    gen = torch.Generator().manual_seed(13 * dim + weighted)
    st, _ = _single_table(dim, gen)
    sp, _, _, _ = bags(gen, weighted, BATCH, DEV)
    # Only stored keys: for a missing plain key the single-table kernel
    # reads default row key % dvd, while the group formula masks the key
    # with 2^key_bits - 1 = 0 at key_bits 0 and reads row 0. The two
    # disagree by design, so fold the missing ids onto stored ones.
    values = sp.values % IDS_PER_TABLE
    uniq, inverse = torch.unique(values, return_inverse=True)
    slots = st.lookup(uniq)
    assert int((slots < 0).sum()) == 0
    assert st.key_bits == 0
    weights = sp.weights.float() if weighted else torch.Tensor()
    comb = torch.tensor([COMBINER_ID[combiner]], dtype=torch.int32,
                        device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        single = st.pooled_lookup(uniq, slots, inverse, sp.offsets,
                                  sp.row_ids(), combiner, sp.weights, dtype)
        group = st.ext.group_pooled_fwd(
            st.values, st.default_values, uniq, slots,
            inverse.to(torch.int32), sp.offsets.to(torch.int32), weights,
            comb, BATCH, 1, st.key_bits, st._no_permission_value(),
            st._use_no_permission(), dtype)
        assert torch.equal(single, group)
