"""Hot-key sweep for the sparse engine's three skew-sensitive kernels.

Times dedup pass A (HbmStorage._dedup_claim), pass C (_dedup_count) and
the pooled-grad scatter on two inputs of identical nnz:

  zipf      the DLRM benchmark batch (8192 x 26 Criteo-like zipf ids)
  distinct  the same shape with ids made all-distinct per table, so every
            count is 1 and any wave-level grouping is pure overhead

A kernel that is bound by hot keys is several times faster on `distinct`
although that input has more unique keys. The scatter is swept over its
group size R. Each figure is the mean of an event-timed loop; `spread` is
max - min over --repeats such loops. The loops launch eagerly, so very
short kernels bottom out at the host launch rate: `floor` rows time the
same calls on a 64-key input.

Run on a GPU box: python tools/scatter_sweep.py
"""
import argparse

import torch

from deeprec_amd.data.synthetic import CriteoSyntheticDataset
from deeprec_amd.embedding.options import EmbeddingVariableOption
from deeprec_amd.ops.hip_backend import HbmStorage


def time_fn(fn, iters=100):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000.0  # us


def report(label, fn, repeats):
    ts = sorted(time_fn(fn) for _ in range(repeats))
    print(f"  {label:<28} median {ts[len(ts) // 2]:7.1f} us   "
          f"spread {ts[-1] - ts[0]:5.1f} us   runs "
          + " ".join(f"{t:.1f}" for t in ts), flush=True)


def make_inputs(batch, n_tables, dev):
    ds = CriteoSyntheticDataset(batch_size=batch, device=dev, seed=1234,
                                matrix_format=True)
    _, ids, _ = ds.next_batch()          # [B, 26] raw ids
    tags = torch.arange(n_tables, device=dev, dtype=torch.int64) << 48
    zipf = (ids.t() + tags.unsqueeze(1)).reshape(-1)  # table-major
    gen = torch.Generator(device="cpu").manual_seed(1234)
    perm = torch.stack([torch.randperm(batch, generator=gen)
                        for _ in range(n_tables)]).to(dev)
    distinct = (perm + tags.unsqueeze(1)).reshape(-1)
    floor = zipf[:64].clone()
    return {"zipf": zipf, "distinct": distinct, "floor": floor}


def sweep_input(name, keys, batch, n_tables, dim, repeats):
    dev = keys.device
    nnz = keys.numel()
    st = HbmStorage(dim, EmbeddingVariableOption(init_capacity=1 << 23),
                    device=dev)
    st.enable_graph_mode(expected_entries=1 << 23, expected_slots=1 << 23)
    ext = st.ext

    def claim():
        # as in the captured step: device epoch, bumped before every claim
        ext.bump_epoch(st._epoch_dev, st._step_dev)
        return st._dedup_claim(keys, st._epoch_dev)

    _, _, occ_entry, m_counter = claim()
    m = int(m_counter)
    inverse, counts, rank = st._dedup_count(occ_entry, nnz)
    c = counts[:m]
    print(f"[{name}] nnz={nnz} m={m} max_count={int(c.max())} "
          f"top4={c.topk(min(4, m)).values.tolist()} "
          f"count1={int((c == 1).sum())} "
          f"count>32={int((c > 32).sum())}", flush=True)
    report("pass A (_dedup_claim)", claim, repeats)
    report("pass C (_dedup_count)",
           lambda: st._dedup_count(occ_entry, nnz), repeats)
    if nnz != batch * n_tables:
        return
    # backward on the capture-shaped (nnz-padded) unique rows
    bounds = torch.zeros(nnz + 1, dtype=torch.int32, device=dev)
    bounds[1:] = counts.cumsum(0)
    order = ext.csr_scatter(inverse, rank, bounds, st.error_flag)
    st._check_error()
    row_ids = torch.arange(nnz, dtype=torch.int32, device=dev)
    row_coeff = torch.ones(nnz, device=dev)
    grad = torch.randn(batch, n_tables * dim, device=dev,
                       dtype=torch.bfloat16)
    for r in (4, 8, 16, 32):
        report(f"bwd seg R={r}", lambda: ext.group_pooled_bwd_seg(
            grad, order, inverse, row_ids, torch.Tensor(), row_coeff,
            nnz, batch, n_tables, dim, True, r), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inputs", default="zipf,distinct,floor",
                    help="comma-separated subset of zipf,distinct,floor "
                         "(one at a time under a kernel trace, where the "
                         "kernel names do not tell the inputs apart)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    batch, n_tables, dim = 8192, 26, 16
    inputs = make_inputs(batch, n_tables, dev)
    for name in args.inputs.split(","):
        sweep_input(name, inputs[name], batch, n_tables, dim, args.repeats)


if __name__ == "__main__":
    main()
