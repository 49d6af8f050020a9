"""fp64 reference and error bound for the pooled embedding reads
(k_pooled_fwd / k_group_pooled_fwd in ops/hip/ev_read_kernels.hip), shared
by the tests of every row source. The reference itself needs no GPU.

The kernel computes, per output element, acc = sum_j fl(w_j * v_j) in
fp32 in j order (L products, L - 1 sums that matter), then fl(acc *
coeff) with coeff one or two fp32 operations on the weight sum. Each
rounding is at most 2^-24 relative to a partial result bounded by
sum_j |w_j v_j|, which gives, to first order,
    |out - ref| <= (L + 2) * 2^-24 * coeff * sum_j |w_j v_j|.
A bf16 output adds one more rounding: 2^-8 * |ref| (2^-9 half-ulp plus the
fp32 error above moving the rounding point; 2^-8 covers both).
"""
import torch

IDS_PER_TABLE = 40     # ids 0..39 are stored; 40..44 are missing keys


def bags(gen, weighted, n_rows, device):
    """n_rows bags of 0..5 ids over 0..IDS_PER_TABLE+4 as a RaggedIds on
    `device`, plus the same ids / offsets / weights on the CPU."""
    from deeprec_amd.embedding.ragged import RaggedIds
    lengths = torch.randint(0, 6, (n_rows,), generator=gen)
    lengths[0], lengths[1] = 0, 5        # an empty bag and a full one
    offsets = torch.zeros(n_rows + 1, dtype=torch.int32)
    offsets[1:] = lengths.cumsum(0)
    nnz = int(offsets[-1])
    ids = torch.randint(0, IDS_PER_TABLE + 5, (nnz,), generator=gen)
    ids[0] = IDS_PER_TABLE + 1           # at least one missing key
    w = (torch.rand(nnz, generator=gen) + 0.5) if weighted else None
    return RaggedIds(ids.to(device), offsets.to(device),
                     w.to(device) if weighted else None), ids, offsets, w


def pool_reference(rows_of, ids, offsets, w, combiner):
    """float64 pool over the rows rows_of(ids) gives: (ref, bound term
    coeff * sum |w v|, bag length), each [n_rows, dim] / [n_rows]."""
    n_rows = offsets.numel() - 1
    dim = rows_of(ids[:0]).shape[1]
    ref = torch.zeros(n_rows, dim, dtype=torch.float64)
    mag = torch.zeros(n_rows, dim, dtype=torch.float64)
    lens = torch.zeros(n_rows, dtype=torch.float64)
    for r in range(n_rows):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        if hi == lo:
            continue
        v = rows_of(ids[lo:hi]).double()
        wj = (w[lo:hi].double() if w is not None
              else torch.ones(hi - lo, dtype=torch.float64))
        if combiner == "sum":
            coeff = 1.0
        elif combiner == "mean":
            coeff = 1.0 / float(wj.sum())
        else:
            coeff = 1.0 / float((wj * wj).sum().sqrt())
        ref[r] = (wj[:, None] * v).sum(0) * coeff
        mag[r] = (wj[:, None] * v).abs().sum(0) * coeff
        lens[r] = hi - lo
    return ref, mag, lens


def check_pool(out, ref, mag, lens, label):
    bound = (lens[:, None] + 2) * 2.0 ** -24 * mag
    if out.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (out.cpu().double() - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{label}: max err/bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{label}: err/bound {worst:.3f}"
