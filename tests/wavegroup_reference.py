"""Inputs and exact references for the wave-grouped dedup pass A and the
segmented backward (tests/test_gpu_sparse_wavegroup.py), and
the structure of those inputs computed from their counts alone
(tests/test_sparse_wavegroup_cpu.py). CPU tensors only.

Backward inputs follow test_gpu_sparse_hotkeys.py: integer gradients in
[-4, 4] and weights * coefficients that are multiples of 1/4, so every
contribution is an integer number of quarters and the int64 index_add in
quarter units is the exact result whatever the order of the fp32 additions,
as long as every partial sum stays below 2**24 quarters.
"""
import functools

import torch

BLOCK = 256          # threads per block of the engine kernels
WAVE = 64
PAD_KEY = 2 ** 63 - 1
KEY_BITS = 48        # table tag position of composite keys
R_SWEEP = (4, 8, 16, 32)
SIZES = (1, 7, 129, 1031)


def lanes(dim):
    return 16 if dim >= 16 else 8


def span_of(r, dim):
    """Positions of `order` one block covers per slice."""
    return (BLOCK // lanes(dim)) * r


# --------------------------------------------------------------------------
# backward: count patterns
# --------------------------------------------------------------------------

def patterns(r, span):
    """name -> per-key occurrence counts, in sorted (CSR) order, for R = r
    positions per lane group and `span` positions per block."""
    p = {}
    # a run of exactly one block slice, aligned to it
    p["block_run"] = [1] * span + [span] + [1] * 5
    # cut by group and block edges; over three blocks
    p["long_run_at_5"] = [1] * 5 + [2 * span + 44] + [1] * 7
    # (nearly) every group edge cuts a run
    p["runs_of_r_plus_1"] = [r + 1] * (span // r + 9)
    # two different cut runs meet inside one group of one block: that
    # group has a head of the first and a tail of the second
    p["two_runs_meet"] = [1] * 3 + [2 * r + 4] + [3 * r + 6] + [1] * 4
    # a group lying wholly inside a longer run (one partial, not two)
    p["group_inside_run"] = [1] * 2 + [3 * r] + [1] * 3
    # no cut anywhere: the vote path, plain stores only
    p["all_ones"] = [1] * (2 * span + 37)
    for n in SIZES:
        p[f"nnz{n}"] = _random_counts(n, seed=n)
    p["mixed"] = sum((p[k] for k in ("long_run_at_5", "two_runs_meet",
                                     "runs_of_r_plus_1", "all_ones",
                                     "group_inside_run", "nnz129")), [])
    return p


def _random_counts(nnz, seed):
    """Zipf-like counts adding up to nnz: a hot key of about nnz / 3, a few
    middling ones, count-1 keys in between."""
    gen = torch.Generator().manual_seed(seed)
    counts, left = [], nnz
    hot = max(1, nnz // 3)
    while left > 0:
        pick = int(torch.randint(0, 4, (1,), generator=gen))
        c = (hot, 1, 1, int(torch.randint(2, 20, (1,), generator=gen)))[pick]
        hot = max(1, hot // 2)
        c = min(c, left)
        counts.append(c)
        left -= c
    return counts


def runs_of(counts):
    """[(begin, end)) position range of every key's run."""
    out, pos = [], 0
    for c in counts:
        out.append((pos, pos + c))
        pos += c
    return out


def structure(counts, r, span):
    """What the kernel meets on these counts, from the positions alone."""
    runs = runs_of(counts)
    nnz = runs[-1][1]
    s = dict(nnz=nnz, blocks=-(-nnz // span),
             max_count=max(counts),
             cut_by_group_edge=0, cut_by_block_edge=0,
             merged_to_plain_store=0, single_partial_groups=0,
             head_and_tail_groups=0, blocks_without_cut=0,
             run_is_a_block=0)
    edges_cut = set()
    for b, e in runs:
        inner = [x for x in range((b // r + 1) * r, e, r)]  # b < x < e
        edges_cut.update(inner)
        if inner:
            s["cut_by_group_edge"] += 1
            if any(x % span == 0 for x in inner):
                s["cut_by_block_edge"] += 1
            else:
                s["merged_to_plain_store"] += 1
        # groups [g, g + r) with b < g and g + r < e: cut on both sides
        s["single_partial_groups"] += sum(
            1 for g in inner if g + r < e)
        if b % span == 0 and e - b == span:
            s["run_is_a_block"] += 1
    for g in range(0, nnz, r):
        if g in edges_cut and g + r in edges_cut:
            # a head and a tail of different runs: some run ends inside
            if any(g < e < g + r for _, e in runs):
                s["head_and_tail_groups"] += 1
    for blk in range(s["blocks"]):
        lo, hi = blk * span, (blk + 1) * span
        if not any(lo <= x <= hi for x in edges_cut):
            s["blocks_without_cut"] += 1
    return s


# --------------------------------------------------------------------------
# backward: problems
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bwd_problem(name, r, dim, identity, corrupt=False):
    """Inputs and the exact int64 reference (quarter units) for one count
    pattern. With corrupt: `order` and `inverse` carry a -1 tail of 11
    padded positions, and one occurrence of a count-1 key has an inverse
    just past the output's rows, so that key's row stays zero."""
    counts = patterns(r, span_of(r, dim))[name]
    gen = torch.Generator().manual_seed(
        1000 + 7 * len(counts) + dim + 2 * identity)
    counts_t = torch.tensor(counts)
    m, nnz = len(counts), int(counts_t.sum())
    pad_rows = 37    # capture padding: rows beyond the true m stay zero
    m_rows = m + pad_rows
    sorted_u = torch.repeat_interleave(torch.arange(m), counts_t)
    perm = torch.randperm(nnz, generator=gen)
    inverse = torch.empty(nnz, dtype=torch.int64)
    inverse[perm] = sorted_u          # occurrence perm[k] sits at sorted k
    order = perm.clone()
    n_pad = 11 if corrupt else 0
    n_all = nnz + n_pad
    if identity:
        n_tables = 3 if n_all % 3 == 0 else 1
        batch = n_all // n_tables
        row_ids = torch.arange(n_all)
        weights = None
        row_coeff = torch.ones(n_all)
    else:
        n_tables, batch = 3, 50
        row_ids = torch.randint(0, batch * n_tables, (n_all,), generator=gen)
        pick = torch.tensor([0.5, 1.0, 2.0])
        weights = pick[torch.randint(0, 3, (n_all,), generator=gen)]
        row_coeff = pick[torch.randint(0, 3, (batch * n_tables,),
                                       generator=gen)]
    g_int = torch.randint(-4, 5, (batch, n_tables * dim), generator=gen)
    rid = row_ids[:nnz]
    rows = (rid % batch) * n_tables + rid // batch
    contrib = g_int.reshape(batch * n_tables, dim)[rows]
    if identity:
        scale4 = torch.full((nnz,), 4, dtype=torch.int64)
    else:
        scale4 = (4 * weights[:nnz] * row_coeff[rid]).long()
        assert torch.equal(scale4.float() / 4, weights[:nnz] * row_coeff[rid])
    contrib4 = contrib * scale4[:, None]
    bad_key = None
    if corrupt:
        ones = (counts_t == 1).nonzero().flatten()
        bad_key = int(ones[ones.numel() // 2])
        j_bad = int((inverse == bad_key).nonzero())
        contrib4[j_bad] = 0                       # skipped by the kernel
        inverse_in = torch.cat([inverse, torch.full((n_pad,), -1)])
        inverse_in[j_bad] = m_rows                # first row out of range
        order = torch.cat([order, torch.full((n_pad,), -1)])
    else:
        inverse_in = inverse
    ref4 = torch.zeros(m, dim, dtype=torch.int64)
    ref4.index_add_(0, inverse, contrib4)
    mag4 = torch.zeros(m, dim, dtype=torch.int64)
    mag4.index_add_(0, inverse, contrib4.abs())
    return dict(r=r, dim=dim, m=m, m_rows=m_rows, nnz=nnz, batch=batch,
                n_tables=n_tables, inverse=inverse_in, order=order,
                row_ids=row_ids, weights=weights, row_coeff=row_coeff,
                g_int=g_int, ref4=ref4, mag4=mag4, counts=counts_t,
                bad_key=bad_key)


# --------------------------------------------------------------------------
# pass A: key cases
# --------------------------------------------------------------------------

def _distinct(n, gen, base=1 << 20):
    return (torch.randperm(4 * n + 8, generator=gen)[:n] + base).long()


@functools.lru_cache(maxsize=None)
def key_cases():
    """name -> (keys, kind), kind one of plain / pad / matrix. For matrix
    the keys are the id matrix [batch, n_tables]."""
    gen = torch.Generator().manual_seed(31)
    cases = {}
    # nnz = 200 (3 waves and 8 lanes): one key on 40 lanes of wave 0 and
    # again in wave 1 (two leaders race for the first touch), duplicates
    # among the others, the last wave partial
    pool = _distinct(60, gen)
    k = pool[torch.randint(0, 60, (200,), generator=gen)]
    hot_lanes = torch.randperm(WAVE, generator=gen)[:40]
    k[hot_lanes] = 31337
    k[WAVE + torch.tensor([3, 17, 18, 60])] = 31337
    cases["hot_key_two_waves"] = (k, "plain")
    # one wave of keys that agree below bit 48: 26 table tags over one id
    tags = torch.arange(26, dtype=torch.int64) << KEY_BITS
    k = (tags + 12345)[torch.randint(0, 26, (WAVE,), generator=gen)]
    k[:26] = tags + 12345                  # every tag is present
    cases["equal_below_bit_48"] = (k, "plain")
    # id matrix, batch 5 x 26 tables, one raw id everywhere: 26 keys of
    # count 5, a wave spanning 12 whole tables and part of a 13th
    cases["matrix_same_id"] = (torch.full((5, 26), 4242, dtype=torch.int64),
                               "matrix")
    # pads: lane 0 of wave 0 is a pad and the rest of lanes 0..19 one key
    # with pads inside (its leader is lane 1); wave 1 is all pads; wave 2
    # is partial
    k = pool[torch.randint(0, 60, (2 * WAVE + 30,), generator=gen)]
    k[:20] = 777
    k[[0, 4, 5, 13]] = PAD_KEY
    k[WAVE:2 * WAVE] = PAD_KEY
    k[2 * WAVE + 7] = PAD_KEY
    cases["pads"] = (k, "pad")
    return cases


def composite_keys(ids):
    """Table-major composite keys of an id matrix [batch, n_tables]:
    occurrence t * batch + b is ids[b, t] + (t << KEY_BITS)."""
    n_tables = ids.shape[1]
    tags = torch.arange(n_tables, dtype=torch.int64) << KEY_BITS
    return (ids.t() + tags.unsqueeze(1)).reshape(-1)
