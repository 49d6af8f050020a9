"""Per-shape microbenchmark of the fused-MLP kernels.

Times linear_fwd / linear_dx / linear_dw on each DLRM layer shape, and on
the model-zoo shapes the same kernels serve, with hipEvents: eager loops
of `--iters` calls, median of `--loops` loops, spread = max - min of the
loops. The loops include the bindings' allocation and zero-fill and bottom
out near the host launch rate for the shortest kernels; take kernel-only
figures from a trace of this script where that matters. Run on a GPU box:
    python tools/gemm_sweep.py
"""
import argparse
import statistics

import torch

from deeprec_amd.ops.build_ext import require_extension

SHAPES = [  # (M, N, K)
    # the DLRM MLP layers at batch 8192
    (8192, 512, 16),
    (8192, 256, 512),
    (8192, 64, 256),
    (8192, 16, 64),
    (8192, 512, 368),
    (8192, 256, 512),
    (8192, 1, 256),
    # model zoo: a tall first layer and a short, wide-N one
    (65536, 256, 429),
    (16, 1024, 429),
]


def time_fn(fn, iters, loops):
    """(median, max - min) of `loops` event-timed loops, us per call."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(loops):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1000.0)
    return statistics.median(out), max(out) - min(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--loops", type=int, default=5)
    args = p.parse_args()
    ext = require_extension()
    dev = torch.device("cuda")
    names = ("fwd0", "fwd1", "dx", "dw16", "dw64t")
    print(f"{'M':>6} {'N':>4} {'K':>4} | "
          + " ".join(f"{n:>12}" for n in names) + "  us (spread)")
    tot = [0.0] * len(names)
    for M, N, K in SHAPES:
        A = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        W = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        b = torch.randn(N, device=dev, dtype=torch.float32)
        G = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
        fns = (lambda: ext.linear_fwd(A, W, b, 1, 0),
               lambda: ext.linear_fwd(A, W, b, 1, 1),
               lambda: ext.linear_dx(G, W),
               lambda: ext.linear_dw(G, A, True, 0),
               lambda: ext.linear_dw(G, A, True, 2))
        res = [time_fn(fn, args.iters, args.loops) for fn in fns]
        print(f"{M:>6} {N:>4} {K:>4} | "
              + " ".join(f"{m:7.1f}({s:3.1f})" for m, s in res))
        for i, (m, _) in enumerate(res):
            tot[i] += m
    print(f"{'TOTAL':>16} | " + " ".join(f"{t:12.1f}" for t in tot))


if __name__ == "__main__":
    main()
