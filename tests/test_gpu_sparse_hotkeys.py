"""Hot-key paths of the sparse engine: the wave-grouped dedup passes A and
C and the occurrence-balanced segmented backward.

Every comparison is exact on integers (the idiom of dense_reference.py):
dedup outputs are checked against torch.unique on the CPU, and the
backward runs on integer-valued gradients whose fp32 sums are exact in any
order, against an int64 index_add. One non-integer case checks the
worst-case fp32 summation bound against fp64.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD_KEY = 2 ** 63 - 1
BLOCK = 256  # threads per block of the engine kernels
WAVE = 64


# --------------------------------------------------------------------------
# dedup
# --------------------------------------------------------------------------

def _storage(graph):
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    from deeprec_amd.ops.hip_backend import HbmStorage
    st = HbmStorage(8, EmbeddingVariableOption(init_capacity=8192),
                    device=DEV, generator=torch.Generator().manual_seed(5))
    if graph:
        st.enable_graph_mode(4096, 4096)
    return st


def _distinct(n, gen, base=1 << 20):
    """n distinct keys, scrambled."""
    return (torch.randperm(4 * n + 8, generator=gen)[:n] + base).long()


def _key_cases():
    gen = torch.Generator().manual_seed(11)
    cases = {}
    for nnz in (1, 63, 64, 65, 257):
        pool = _distinct(nnz // 2 + 1, gen)
        cases[f"nnz{nnz}"] = pool[torch.randint(0, pool.numel(), (nnz,),
                                                generator=gen)]
    cases["all_equal_1000"] = torch.full((1000,), 777, dtype=torch.int64)
    cases["all_distinct"] = _distinct(300, gen)
    cases["two_alternating"] = torch.tensor([5, 9] * 96, dtype=torch.int64)
    # one key in lanes 40..63 of wave 0 and lanes 0..20 of wave 1
    k = _distinct(2 * WAVE, gen)
    k[40:WAVE + 21] = 31337
    cases["key_across_wave_edge"] = k
    # one key present in every wave of 5 blocks, at a varying lane, among
    # duplicated others
    nw = 5 * BLOCK // WAVE
    pool = _distinct(200, gen)
    k = pool[torch.randint(0, 200, (5 * BLOCK,), generator=gen)]
    for w in range(nw):
        k[w * WAVE + (7 * w) % WAVE] = 424242
    cases["key_in_every_wave"] = k
    return cases


def _pad_case():
    gen = torch.Generator().manual_seed(12)
    pool = _distinct(40, gen)
    k = pool[torch.randint(0, 40, (3 * WAVE + 9,), generator=gen)]
    k[[0, 31, 63]] = PAD_KEY          # lanes 0, 31, 63 of wave 0
    k[WAVE:2 * WAVE] = PAD_KEY        # a whole wave of pads
    return k


_KEY_CASES = _key_cases()
_KEY_CASES["pads"] = _pad_case()


def _dedup_step(st, keys, graph, pad):
    """Passes A, C, B through the storage's own entry points; returns CPU
    tensors (m, uniq, inverse, counts, rank, slots)."""
    nnz = keys.numel()
    if graph:
        st.ext.bump_epoch(st._epoch_dev, st._step_dev)
        uniq_buf, centry, occ, m_counter = st._dedup_claim(keys,
                                                           st._epoch_dev)
        inverse, counts, rank = st._dedup_count(
            occ, nnz, pad_keys=keys if pad else None)
        slots = st._dedup_admit(centry, uniq_buf, counts, m_dev=m_counter)
        m = int(m_counter)
    else:
        st._ensure_capacity(nnz)
        st._epoch += 1
        uniq_buf, centry, occ, m_counter = st._dedup_claim(keys)
        m = int(m_counter)
        inverse, counts, rank = st._dedup_count(
            occ, m, pad_keys=keys if pad else None)
        slots = st._dedup_admit(centry[:m], uniq_buf[:m], counts, step=1)
    st._check_error()
    return m, uniq_buf, inverse, counts, rank, slots


def _check_dedup(st, keys_dev, out):
    m, uniq_buf, inverse, counts, rank, slots = out
    keys = keys_dev.cpu()
    nnz = keys.numel()
    uniq, inv, cnt, rk, sl = (t.cpu() for t in
                              (uniq_buf, inverse, counts, rank, slots))
    ref_u, ref_c = torch.unique(keys, return_counts=True)
    assert m == ref_u.numel()
    assert torch.equal(torch.sort(uniq[:m]).values, ref_u)
    real = keys != PAD_KEY
    # pass C only sees pads as pads in the pad variant; without pads in
    # the input `real` is all-true
    assert bool((inv[~real] == -1).all()) and bool((rk[~real] == 0).all())
    inv_r = inv[real].long()
    assert bool((inv_r >= 0).all()) and bool((inv_r < m).all())
    assert torch.equal(uniq[inv_r], keys[real])
    # counts under the key -> compact-index mapping; pads count nothing
    want = torch.zeros(cnt.numel(), dtype=torch.int64)
    want.index_add_(0, inv_r, torch.ones_like(inv_r))
    assert torch.equal(cnt.long(), want)          # includes the padded tail
    pos = torch.searchsorted(ref_u, uniq[:m])
    ref_cnt = ref_c[pos].clone()
    ref_cnt[uniq[:m] == PAD_KEY] = 0
    assert torch.equal(cnt[:m].long(), ref_cnt)
    assert bool((cnt[m:] == 0).all())
    # the ranks of every key's occurrences are exactly {0 .. count-1}
    rk_r = rk[real].long()
    by = torch.argsort(inv_r * (nnz + 1) + rk_r)
    bounds = torch.zeros(cnt.numel() + 1, dtype=torch.int64)
    bounds[1:] = cnt.long().cumsum(0)
    n_real = int(real.sum())
    assert torch.equal(rk_r[by],
                       torch.arange(n_real) - bounds[inv_r[by]])
    # admission: no filter here, so every real key holds a slot
    is_pad_u = uniq[:m] == PAD_KEY
    assert bool((sl[:m][~is_pad_u] >= 0).all())
    assert bool((sl[:m][is_pad_u] == -1).all())
    assert bool((sl[m:] == -1).all())
    # CSR order over the real occurrences: a direct scatter by rank
    if n_real:
        b32 = bounds.to(torch.int32).to(DEV)
        order = st.ext.csr_scatter(inverse[real.to(DEV)].contiguous(),
                                   rank[real.to(DEV)].contiguous(), b32,
                                   st.error_flag)
        st._check_error()
        order = order.cpu().long()
        assert torch.equal(torch.sort(order).values, torch.arange(n_real))
        sorted_u = inv_r[order]
        assert bool((sorted_u[1:] >= sorted_u[:-1]).all())


# PAD_KEY only exists on the owner side of the padded exchange, which
# always runs with the device epoch (eager pass B has no pad handling)
_DEDUP_PARAMS = [(c, g) for c in _KEY_CASES for g in (False, True)
                 if g or c != "pads"]


@pytest.mark.parametrize(
    "case,graph", _DEDUP_PARAMS,
    ids=[f"{c}-{'device_epoch' if g else 'eager'}"
         for c, g in _DEDUP_PARAMS])
def test_dedup_matches_unique(case, graph):
    keys = _KEY_CASES[case].to(DEV)
    pad = case == "pads"
    st = _storage(graph)
    # the second step finds every key already in the table, stamped with
    # the previous epoch: the stale-epoch claim path
    for _ in range(2):
        _check_dedup(st, keys, _dedup_step(st, keys, graph, pad))


def test_pass_c_entries_equal_in_low_bits():
    """Entries that differ only above bit 14: the wave grouping cannot stop
    after its first rounds of low bits and must still group exactly."""
    gen = torch.Generator().manual_seed(13)
    n_keys, nnz, shift = 40, 300, 14
    comp = torch.randint(0, n_keys, (nnz,), generator=gen)
    occ_entry = (comp << shift).to(DEV)
    ht_compact = torch.zeros(n_keys << shift, dtype=torch.int32)
    ht_compact[torch.arange(n_keys) << shift] = torch.arange(
        n_keys, dtype=torch.int32)
    inverse, counts, rank = _ext().ht_dedup_c(None, occ_entry,
                                              ht_compact.to(DEV), n_keys)
    inverse, counts, rank = inverse.cpu(), counts.cpu(), rank.cpu()
    assert torch.equal(inverse.long(), comp)
    assert torch.equal(counts.long(), torch.bincount(comp, minlength=n_keys))
    by = torch.argsort(comp * (nnz + 1) + rank.long())
    bounds = torch.zeros(n_keys + 1, dtype=torch.int64)
    bounds[1:] = counts.long().cumsum(0)
    assert torch.equal(rank.long()[by], torch.arange(nnz) - bounds[comp[by]])


# --------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------

def _lanes(dim):
    return 16 if dim >= 16 else 8


def _seg_counts(R, span, multiple_of):
    """Per-key occurrence counts whose sorted runs hit every edge of the
    segmented backward for R positions per lane group and `span`
    positions per block. Returns (counts, marks) where marks names the
    key index of each constructed situation."""
    counts, marks = [], {}
    pos = 0

    def put(c, name=None):
        nonlocal pos
        if name:
            marks[name] = (len(counts), pos)
        counts.append(c)
        pos += c

    def align(target, mod):
        while pos % mod != target:
            put(1)

    put(1, "count_1")
    put(R, "exactly_R_unaligned")
    align(0, R)
    put(R, "exactly_R_aligned")
    put(R - 1, "R_minus_1")
    put(R + 1, "R_plus_1")
    align(R - 1, R)
    put(3, "starts_on_last_of_group")
    align(R - 2, R)
    put(3, "ends_on_first_of_group")
    align(span - 1, span)
    put(span + 2, "spans_three_blocks")
    put(2 * R + 3, "covers_whole_groups")
    while (pos + 5) % multiple_of != 0 or (pos + 5) % R == 0:
        put(1)
    put(5, "last_key")
    return counts, marks


@functools.lru_cache(maxsize=None)
def _bwd_problem(dim, identity):
    """Inputs and the exact int64 reference, built once per shape."""
    ext = _ext()
    R = int(ext.BWD_SEG_R)
    span = (BLOCK // _lanes(dim)) * R
    n_tables = 3
    counts, marks = _seg_counts(R, span, n_tables)
    gen = torch.Generator().manual_seed(100 + dim + identity)
    counts_t = torch.tensor(counts)
    m, nnz = len(counts), int(counts_t.sum())
    # construction self-check
    assert nnz % R != 0 and nnz % n_tables == 0
    k, p = marks["starts_on_last_of_group"]
    assert p % R == R - 1
    k, p = marks["ends_on_first_of_group"]
    assert (p + counts[k] - 1) % R == 0
    k, p = marks["spans_three_blocks"]
    assert (p + counts[k] - 1) // span - p // span == 2
    k, p = marks["exactly_R_aligned"]
    assert p % R == 0 and counts[k] == R
    assert marks["last_key"][0] == m - 1

    sorted_u = torch.repeat_interleave(torch.arange(m), counts_t)
    perm = torch.randperm(nnz, generator=gen)
    inverse = torch.empty(nnz, dtype=torch.int64)
    inverse[perm] = sorted_u          # occurrence perm[k] sits at sorted k
    order = perm.clone()
    if identity:
        batch = nnz // n_tables
        row_ids = torch.arange(nnz)
        weights = None
        row_coeff = torch.ones(nnz)
    else:
        batch = 50
        row_ids = torch.randint(0, batch * n_tables, (nnz,), generator=gen)
        pick = torch.tensor([0.5, 1.0, 2.0])
        weights = pick[torch.randint(0, 3, (nnz,), generator=gen)]
        row_coeff = pick[torch.randint(0, 3, (batch * n_tables,),
                                       generator=gen)]
    g_int = torch.randint(-4, 5, (batch, n_tables * dim), generator=gen)
    # int64 reference in quarter units (weights * coeff is a multiple of
    # 1/4, so 4 * contribution is an integer)
    rid = row_ids
    rows = (rid % batch) * n_tables + rid // batch
    contrib = g_int.reshape(batch * n_tables, dim)[rows]
    if identity:
        scale4 = torch.full((nnz,), 4, dtype=torch.int64)
    else:
        scale4 = (4 * weights * row_coeff[rid]).long()
        assert torch.equal(scale4.float() / 4, weights * row_coeff[rid])
    ref4 = torch.zeros(m, dim, dtype=torch.int64)
    ref4.index_add_(0, inverse, contrib * scale4[:, None])
    return dict(R=R, m=m, nnz=nnz, batch=batch, n_tables=n_tables,
                inverse=inverse, order=order, row_ids=row_ids,
                weights=weights, row_coeff=row_coeff, g_int=g_int,
                ref4=ref4, counts=counts_t)


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _run_bwd(p, grad, dim, identity, m_rows, r=0):
    i32 = dict(dtype=torch.int32, device=DEV)
    w = (p["weights"].to(DEV) if p["weights"] is not None
         else torch.Tensor())
    out = _ext().group_pooled_bwd_seg(
        grad.to(DEV).contiguous(), p["order"].to(**i32),
        p["inverse"].to(**i32), p["row_ids"].to(**i32), w,
        p["row_coeff"].to(DEV), m_rows, p["batch"], p["n_tables"], dim,
        identity, r)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("identity", [True, False],
                         ids=["identity", "weighted"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("dim", [8, 16])
def test_bwd_seg_exact(dim, dtype, identity):
    p = _bwd_problem(dim, identity)
    pad_rows = 37   # capture padding: rows beyond the true m stay zero
    out = _run_bwd(p, p["g_int"].to(dtype), dim, identity, p["m"] + pad_rows)
    assert out.shape == (p["m"] + pad_rows, dim)
    assert torch.equal((out[:p["m"]].double() * 4).long(), p["ref4"])
    assert torch.equal(out[:p["m"]].double() * 4, p["ref4"].double())
    assert bool((out[p["m"]:] == 0).all())


@pytest.mark.parametrize("r", [4, 8, 16, 32])
def test_bwd_seg_every_r_exact(r):
    """The other group sizes exist for the sweep tool; same exact result."""
    p = _bwd_problem(16, True)
    out = _run_bwd(p, p["g_int"].to(torch.bfloat16), 16, True, p["m"], r)
    assert torch.equal(out.double() * 4, p["ref4"].double())


def test_bwd_seg_fp32_rounding_bound():
    """Non-integer gradients against fp64: per element the error is at
    most count * 2^-24 * sum|contribution| over that key, the worst case
    of fp32 summation in any order."""
    dim = 16
    p = _bwd_problem(dim, False)
    gen = torch.Generator().manual_seed(9)
    grad = torch.randn(p["batch"], p["n_tables"] * dim, generator=gen)
    out = _run_bwd(p, grad, dim, False, p["m"]).double()
    rid = p["row_ids"]
    rows = (rid % p["batch"]) * p["n_tables"] + rid // p["batch"]
    scale = (p["weights"] * p["row_coeff"][rid]).double()
    contrib = grad.double().reshape(-1, dim)[rows] * scale[:, None]
    ref = torch.zeros(p["m"], dim, dtype=torch.float64)
    ref.index_add_(0, p["inverse"], contrib)
    mag = torch.zeros(p["m"], dim, dtype=torch.float64)
    mag.index_add_(0, p["inverse"], contrib.abs())
    bound = p["counts"].double()[:, None] * 2.0 ** -24 * mag
    err = (out - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"max err/bound = {worst:.3f}")
    assert bool((err <= bound).all())


def test_captured_dedup_backward_replays():
    """dedup_lookup_capture -> _prep_backward -> backward in one small
    hipGraph, replayed on three different batches: every replay must
    re-zero counts and the grad buffer and advance the epoch (recorded
    memset nodes once did not replay)."""
    from deeprec_amd.embedding.collection import EmbeddingCollection
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    batch, n_tables, dim = 200, 3, 16
    nnz = batch * n_tables
    coll = EmbeddingCollection(
        "hot", ["a", "b", "c"], dim, device=DEV,
        ev_option=EmbeddingVariableOption(init_capacity=8192))
    st = coll.storage
    st.enable_graph_mode(4096, 4096)
    coll.graph_mode = True
    row_ids = torch.arange(nnz, dtype=torch.int32, device=DEV)
    row_coeff = torch.ones(nnz, device=DEV)
    tags = (torch.arange(n_tables, dtype=torch.int64) << 48) \
        .repeat_interleave(batch)

    gen = torch.Generator().manual_seed(21)

    def make_batch(i):
        # zipf-like: a few hot ids plus a uniform tail, other ids each time
        hot = torch.randint(0, 4, (nnz,), generator=gen) + 10 * i
        cold = torch.randint(0, 500, (nnz,), generator=gen) + 1000 * i
        ids = torch.where(torch.rand(nnz, generator=gen) < 0.5, hot, cold)
        g = torch.randint(-4, 5, (batch, n_tables * dim), generator=gen)
        return ids + tags, g

    s_keys = torch.zeros(nnz, dtype=torch.int64, device=DEV)
    s_grad = torch.zeros(batch, n_tables * dim, dtype=torch.bfloat16,
                         device=DEV)

    def step():
        d = st.dedup_lookup_capture(s_keys)
        order, bounds = coll._prep_backward(d.inverse, d.counts, d.rank)
        gu = coll._backward(s_grad, order, bounds, d.inverse, row_ids, None,
                            row_coeff, nnz, batch, identity_rows=True)
        return d.uniq, d.inverse, gu, d.m_dev

    k0, g0 = make_batch(0)
    s_keys.copy_(k0)
    s_grad.copy_(g0)
    step()                      # eager warm-up of every kernel
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        uniq, inverse, gu, m_dev = step()
    torch.cuda.synchronize()
    for i in range(1, 4):
        keys, g = make_batch(i)
        s_keys.copy_(keys)
        s_grad.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        st._check_error()
        m = int(m_dev)
        assert m == torch.unique(keys).numel()
        inv = inverse.cpu().long()
        assert torch.equal(uniq.cpu()[inv], keys)
        j = torch.arange(nnz)
        rows = (j % batch) * n_tables + j // batch
        ref = torch.zeros(nnz, dim, dtype=torch.int64)
        ref.index_add_(0, inv, g.reshape(-1, dim)[rows])
        out = gu.cpu().double()
        assert torch.equal(out, ref.double())
        assert bool((out[m:] == 0).all())
