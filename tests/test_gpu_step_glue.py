"""The captured step's sparse-lookup glue as HIP kernels: csr_bounds (int32
exclusive scan), pass A reading the id matrix, the k_dedup_begin prologue,
and lookup_matrix end to end against the formulation it replaced.
Everything here is integers or exactly-summable floats, so comparisons
are exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _storage(graph=False, seed=5):
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    from deeprec_amd.ops.common import KEY_BITS
    from deeprec_amd.ops.hip_backend import HbmStorage
    st = HbmStorage(8, EmbeddingVariableOption(init_capacity=8192),
                    device=DEV, generator=torch.Generator().manual_seed(seed))
    st.key_bits = KEY_BITS
    if graph:
        st.enable_graph_mode(4096, 4096)
    return st


# --------------------------------------------------------------------------
# csr_bounds
# --------------------------------------------------------------------------

def _bounds_ref(counts):
    ref = torch.zeros(counts.numel() + 1, dtype=torch.int64)
    ref[1:] = counts.long().cumsum(0)
    return ref.to(torch.int32)


def _scan_sizes():
    ext = _ext()
    tile, cap = ext.CSR_SCAN_TILE, ext.CSR_SCAN_MAX_BLOCKS
    return tile, [0, 1, tile - 1, tile, tile + 1, 3 * tile + 7,
                  tile * cap + tile + 3]      # the last: past the block cap


def test_csr_bounds_equals_cumsum():
    tile, sizes = _scan_sizes()
    gen = torch.Generator().manual_seed(0)
    for m in sizes:
        counts = torch.randint(0, 6, (m,), generator=gen, dtype=torch.int32)
        out = _ext().csr_bounds(counts.to(DEV))
        assert out.dtype == torch.int32 and out.shape == (m + 1,)
        assert torch.equal(out.cpu(), _bounds_ref(counts)), m


def test_csr_bounds_with_a_zero_tail():
    """Capture padding: the counts past the unique count are zero, so the
    bounds stay at nnz over the whole tail (several tiles of it)."""
    tile, _ = _scan_sizes()
    m = 3 * tile + 7
    gen = torch.Generator().manual_seed(1)
    counts = torch.randint(1, 9, (m,), generator=gen, dtype=torch.int32)
    counts[tile // 2 + 3:] = 0
    out = _ext().csr_bounds(counts.to(DEV)).cpu()
    assert torch.equal(out, _bounds_ref(counts))
    assert bool((out[tile // 2 + 3:] == int(counts.sum())).all())


def test_csr_bounds_repeats_and_rejects_other_dtypes():
    counts = torch.randint(0, 6, (5000,), dtype=torch.int32).to(DEV)
    assert torch.equal(_ext().csr_bounds(counts), _ext().csr_bounds(counts))
    with pytest.raises(RuntimeError):
        _ext().csr_bounds(counts.long())


# --------------------------------------------------------------------------
# pass A from the id matrix
# --------------------------------------------------------------------------

def _composite(ids):
    from deeprec_amd.ops.common import KEY_BITS
    batch, n = ids.shape
    tags = (torch.arange(n, dtype=torch.int64, device=ids.device)
            << KEY_BITS).repeat_interleave(batch)
    return ids.t().reshape(-1) + tags


@pytest.mark.parametrize("batch,n", [(1, 1), (3, 26), (257, 2), (64, 26)])
def test_dedup_a_matrix_matches_the_key_array_path(batch, n):
    gen = torch.Generator().manual_seed(batch * 31 + n)
    # a small id range: repeats within a table, and the same raw id under
    # several tables (distinct composite keys)
    ids = torch.randint(0, max(2, batch // 2), (batch, n),
                        generator=gen).to(DEV)
    keys = _composite(ids)
    nnz = keys.numel()

    st_m, st_k = _storage(), _storage()
    st_m._epoch += 1
    st_k._epoch += 1
    uniq_m, _, occ_m, m_m = st_m._dedup_claim(ids, matrix=True)
    uniq_k, _, occ_k, m_k = st_k._dedup_claim(keys)
    st_m._check_error()
    st_k._check_error()
    m = int(m_m)
    assert m == int(m_k)
    assert int(st_m.entry_counter) == int(st_k.entry_counter) == m

    ref_u = torch.unique(keys)
    assert m == ref_u.numel()
    assert torch.equal(torch.sort(uniq_m[:m])[0], ref_u)
    assert torch.equal(torch.sort(uniq_k[:m])[0], ref_u)
    # claim order is decided by atomics: compare through the compact ids
    assert occ_m.shape == (nnz,)
    assert torch.equal(uniq_m[st_m.ht_compact[occ_m].long()], keys)
    assert torch.equal(uniq_k[st_k.ht_compact[occ_k].long()], keys)


def test_dedup_a_matrix_rejects_a_transposed_view():
    st = _storage()
    ids = torch.randint(0, 9, (4, 3), device=DEV)
    with pytest.raises(RuntimeError):
        st._dedup_claim(ids.t(), matrix=True)


# --------------------------------------------------------------------------
# k_dedup_begin under capture
# --------------------------------------------------------------------------

def test_dedup_begin_resets_per_replay():
    """The memset-node regression guard: counts and the unique counter are
    zeroed by a kernel inside the captured step, so nothing accumulates
    across replays."""
    batch, n = 64, 3
    gen = torch.Generator().manual_seed(9)
    batches = [torch.randint(0, 20 + 15 * i, (batch, n), generator=gen)
               for i in range(4)]
    st = _storage(graph=True)
    sids = batches[0].to(DEV)
    st.dedup_lookup_capture_matrix(sids)        # warm up outside capture
    torch.cuda.synchronize()
    epoch0 = int(st._epoch_dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d = st.dedup_lookup_capture_matrix(sids)
    torch.cuda.synchronize()
    for i, ids in enumerate(batches[1:3] + batches[1:2]):
        sids.copy_(ids)
        g.replay()
        torch.cuda.synchronize()
        st._check_error()
        m_ref = torch.unique(_composite(ids)).numel()
        assert int(d.m_dev) == m_ref, i
        assert int(d.counts.sum()) == batch * n, i
        assert int(d.counts[:m_ref].sum()) == batch * n, i
        assert bool((d.counts[m_ref:] == 0).all()), i
    assert int(st._epoch_dev) == epoch0 + 3     # one bump per replay


def test_dedup_begin_epoch_only():
    st = _storage(graph=True)
    m_counter = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    counts = torch.full((1030,), 3, dtype=torch.int32, device=DEV)
    e0, s0 = int(st._epoch_dev), int(st._step_dev)
    st.ext.dedup_begin(st._epoch_dev, None, m_counter, counts)
    assert (int(st._epoch_dev), int(st._step_dev)) == (e0 + 1, s0)
    assert int(m_counter) == 0 and not bool(counts.any())
    counts.fill_(3)
    st.ext.dedup_begin(st._epoch_dev, st._step_dev, m_counter, counts[:1027])
    assert (int(st._epoch_dev), int(st._step_dev)) == (e0 + 2, s0 + 1)
    assert not bool(counts[:1027].any()) and bool((counts[1027:] == 3).all())


# --------------------------------------------------------------------------
# lookup_matrix end to end
# --------------------------------------------------------------------------

def _collection(seed=5):
    from deeprec_amd.embedding.collection import EmbeddingCollection
    coll = EmbeddingCollection("glue/sparse", ["a", "b", "c"], 16,
                               device=DEV,
                               generator=torch.Generator().manual_seed(seed))
    coll.storage.enable_graph_mode(4096, 4096)
    coll.graph_mode = True
    return coll


def _per_key(uniq, grad, m):
    order = torch.argsort(uniq[:m])
    return uniq[:m][order], grad[:m][order]


def test_lookup_matrix_equals_the_parent_formulation():
    batch, n, dim = 64, 3, 16
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 40, (batch, n), generator=gen).to(DEV)
    # integer-valued upstream gradient: fp32 sums are exact in any order
    w = torch.randint(-8, 9, (batch, n * dim), generator=gen).float().to(DEV)

    coll = _collection()
    out = coll.lookup_matrix(ids)
    (out * w).sum().backward()
    (slots, uniq, grad), = coll.consume_grads()
    coll.storage._check_error()
    assert coll._anchor.grad is None

    # the formulation this replaced, from the existing bindings: key array
    # by transpose+add, key-array pass A, torch.cumsum bounds
    ref = _collection()
    st = ref.storage
    values_cat, offsets, row_ids, row_coeff = ref.matrix_inputs(ids)
    assert torch.equal(values_cat, _composite(ids))
    d = st.dedup_lookup_capture(values_cat)
    bounds = torch.zeros(d.counts.numel() + 1, dtype=torch.int32, device=DEV)
    bounds[1:] = d.counts.cumsum(0)
    order = st.ext.csr_scatter(d.inverse, d.rank, bounds, st.error_flag)
    out_ref = ref._forward(d.uniq, d.slots, d.inverse, offsets, None, batch,
                           None)
    grad_ref = ref._backward(w, order, bounds, d.inverse, row_ids, None,
                             row_coeff, d.uniq.numel(), batch, True)
    st._check_error()

    m = int(d.m_dev)
    assert m == torch.unique(values_cat).numel()
    assert torch.equal(out, out_ref)
    ku, gu = _per_key(uniq, grad, m)
    kr, gr = _per_key(d.uniq, grad_ref, m)
    assert torch.equal(ku, kr)
    assert torch.equal(gu, gr)
    assert bool(gu.any())
