"""Dedup pass A with one probe per distinct key of a wave, and the segmented
backward on the run layouts a combine of cut-run partials has to get right
(runs cut by group and block edges, a group inside a run, two cut runs
meeting in one group, no cut at all).

Inputs, exact references and what each case is built to meet are in
wavegroup_reference.py; test_sparse_wavegroup_cpu.py proves, without a GPU,
that every structural situation occurs and that every sum is exact in fp32
in any order. So every comparison here is exact: no tolerance, no row left
out.
"""
import pytest
import torch

from tests import wavegroup_reference as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMPTY_KEY = -(2 ** 63)


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


# --------------------------------------------------------------------------
# pass A
# --------------------------------------------------------------------------

def _storage(graph):
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    from deeprec_amd.ops.hip_backend import HbmStorage
    st = HbmStorage(8, EmbeddingVariableOption(init_capacity=2048),
                    device=DEV, generator=torch.Generator().manual_seed(5))
    st.key_bits = W.KEY_BITS
    if graph:
        st.enable_graph_mode(1024, 1024)
    return st


def _claim(st, keys, kind, graph, new_epoch=True):
    """Pass A through the storage's entry point, under a new epoch or once
    more under the current one. -> (uniq_buf, occ_entry, m)."""
    nnz = keys.numel()
    kw = dict(pad=kind == "pad", matrix=kind == "matrix")
    if graph:
        if new_epoch:
            st.ext.bump_epoch(st._epoch_dev, st._step_dev)
        uniq, _, occ, m_counter = st._dedup_claim(keys, st._epoch_dev, **kw)
    else:
        if new_epoch:
            st._ensure_capacity(nnz)
            st._epoch += 1
        uniq, _, occ, m_counter = st._dedup_claim(keys, **kw)
    st._check_error()
    return uniq.cpu(), occ.cpu(), int(m_counter)


def _check_claim(st, flat, kind, uniq, occ, m):
    """flat: the occurrences' keys on the CPU, in occurrence order."""
    real = flat != W.PAD_KEY
    ref_u, ref_c = torch.unique(flat[real], return_counts=True)
    ht_keys, ht_compact = st.ht_keys.cpu(), st.ht_compact.cpu()
    assert m == ref_u.numel()
    assert torch.equal(torch.sort(uniq[:m]).values, ref_u)
    assert bool((occ[~real] == -1).all())
    e = occ[real]
    assert bool((e >= 0).all()) and bool((e < ht_keys.numel()).all())
    assert torch.equal(ht_keys[e], flat[real])
    c = ht_compact[e].long()
    assert bool((c >= 0).all()) and bool((c < m).all())
    assert torch.equal(uniq[c], flat[real])
    assert not bool((ht_keys == W.PAD_KEY).any())
    # pass C on these entries: inverse and exact counts
    occ_dev = occ.to(DEV)
    inverse, counts, _ = st._dedup_count(
        occ_dev, flat.numel(),
        pad_keys=flat.to(DEV) if kind == "pad" else None)
    inv, cnt = inverse.cpu().long(), counts.cpu().long()
    assert bool((inv[~real] == -1).all())
    assert torch.equal(uniq[inv[real]], flat[real])
    assert torch.equal(cnt[:m], ref_c[torch.searchsorted(ref_u, uniq[:m])])
    assert bool((cnt[m:] == 0).all())
    return ref_u.numel()


@pytest.mark.parametrize("graph", [False, True],
                         ids=["eager", "device_epoch"])
@pytest.mark.parametrize("case", list(W.key_cases()))
def test_pass_a(case, graph):
    keys_cpu, kind = W.key_cases()[case]
    flat = W.composite_keys(keys_cpu) if kind == "matrix" else keys_cpu
    keys = keys_cpu.to(DEV)
    st = _storage(graph)
    assert int(st.entry_counter) == 0
    # fresh table: every leader claims its entry by CAS
    uniq, occ, m = _claim(st, keys, kind, graph)
    n_keys = _check_claim(st, flat, kind, uniq, occ, m)
    assert int(st.entry_counter) == n_keys
    if case == "matrix_same_id":
        assert m == 26
    # the same keys under the same epoch: found and already stamped, so
    # nobody is a first toucher and the entries are the same
    _, occ2, m2 = _claim(st, keys, kind, graph, new_epoch=False)
    assert m2 == 0 and torch.equal(occ2, occ)
    # and under the next epoch: found, stale stamp, claimed again
    uniq3, occ3, m3 = _claim(st, keys, kind, graph)
    assert torch.equal(occ3, occ)
    _check_claim(st, flat, kind, uniq3, occ3, m3)
    assert int(st.entry_counter) == n_keys
    # the occupied entries are exactly the distinct keys
    assert int((st.ht_keys != EMPTY_KEY).sum()) == n_keys


def test_pass_a_matrix_matches_composite_keys():
    """The id-matrix call against the plain call on the composite keys it
    stands for, each on a table of its own."""
    ids, _ = W.key_cases()["matrix_same_id"]
    flat = W.composite_keys(ids)
    st_m, st_p = _storage(True), _storage(True)
    uniq_m, occ_m, m_m = _claim(st_m, ids.to(DEV), "matrix", True)
    uniq_p, occ_p, m_p = _claim(st_p, flat.to(DEV), "plain", True)
    assert m_m == m_p == 26
    _check_claim(st_m, flat, "matrix", uniq_m, occ_m, m_m)
    _check_claim(st_p, flat, "plain", uniq_p, occ_p, m_p)
    # the same keys behind the same occurrences, and the same table content
    # (which entry a key claims may depend on who wins a shared probe path)
    assert torch.equal(st_m.ht_keys.cpu()[occ_m], st_p.ht_keys.cpu()[occ_p])
    assert torch.equal(torch.sort(st_m.ht_keys).values,
                       torch.sort(st_p.ht_keys).values)
    assert torch.equal(torch.sort(uniq_m[:26]).values,
                       torch.sort(uniq_p[:26]).values)


# --------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------

def _run_bwd(p, dtype, r=0):
    i32 = dict(dtype=torch.int32, device=DEV)
    w = (p["weights"].to(DEV) if p["weights"] is not None
         else torch.Tensor())
    out = _ext().group_pooled_bwd_seg(
        p["g_int"].to(dtype).to(DEV).contiguous(), p["order"].to(**i32),
        p["inverse"].to(**i32), p["row_ids"].to(**i32), w,
        p["row_coeff"].to(DEV), p["m_rows"], p["batch"], p["n_tables"],
        p["dim"], p["weights"] is None, r)
    torch.cuda.synchronize()
    return out.cpu()


def _check_bwd(p, out):
    assert out.shape == (p["m_rows"], p["dim"])
    got4 = out[:p["m"]].double() * 4
    assert torch.equal(got4, p["ref4"].double())
    assert bool((out[p["m"]:] == 0).all())


def test_committed_r():
    assert int(_ext().BWD_SEG_R) == 8   # what the CPU preconditions assume


_PATTERNS = list(W.patterns(8, W.span_of(8, 16)))


@pytest.mark.parametrize("identity", [True, False],
                         ids=["identity", "weighted"])
@pytest.mark.parametrize("dim", [8, 16])
@pytest.mark.parametrize("name", _PATTERNS)
def test_bwd_patterns_exact(name, dim, identity):
    p = W.bwd_problem(name, 8, dim, identity)
    _check_bwd(p, _run_bwd(p, torch.bfloat16))


@pytest.mark.parametrize("identity", [True, False],
                         ids=["identity", "weighted"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("dim", [8, 16, 24, 32])
def test_bwd_shapes_and_types_exact(dim, dtype, identity):
    p = W.bwd_problem("mixed", 8, dim, identity)
    _check_bwd(p, _run_bwd(p, dtype))


@pytest.mark.parametrize("identity", [True, False],
                         ids=["identity", "weighted"])
@pytest.mark.parametrize("dim", [8, 24])
def test_bwd_corrupt_and_padded_exact(dim, identity):
    """A -1 tail on order and inverse, and one inverse past the output's
    rows: skipped, its key's row and the padding rows stay zero."""
    p = W.bwd_problem("mixed", 8, dim, identity, True)
    out = _run_bwd(p, torch.bfloat16)
    _check_bwd(p, out)
    assert bool((out[p["bad_key"]] == 0).all())


@pytest.mark.parametrize("r", W.R_SWEEP)
def test_bwd_every_r_exact(r):
    p = W.bwd_problem("mixed", r, 16, True)
    _check_bwd(p, _run_bwd(p, torch.bfloat16, r))
