"""Microbenchmark of the DLRM pair-dot interaction kernels alone.

Times interact_cat_fwd and interact_cat_bwd at the flagship shape
(B = 8192, Fe = 26, D = 16, P_pad = 352) with the scalar kernels
(variant 1) and the MFMA kernels (variant 2), calling the extension
directly. Device events around each timed window; every configuration is
warmed up first; the timed loops visit the configurations in turn, so
drift of the machine lands on all of them alike. Reported: median over
`--loops` loops of the mean over `--iters` calls, the spread (max - min)
of the loops, the bytes the call must move (computed from the shapes: each
operand read once, each result written once) and bytes over the median.
Run on a GPU box:
    python -m tools.bench_interact
"""
import argparse
import statistics

import torch

from deeprec_amd.ops.build_ext import require_extension

VARIANTS = [(1, "scalar"), (2, "mfma")]
BF16 = 2


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--features", type=int, default=26)
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--loops", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_interact needs a GPU"
    dev = torch.device("cuda", 0)
    ext = require_extension()
    torch.manual_seed(0)
    b, fe, d = args.batch, args.features, 16
    f = fe + 1
    pairs = f * (f - 1) // 2
    p_pad = (pairs + 15) & ~15
    bot = torch.randn(b, d, device=dev).to(torch.bfloat16)
    emb = torch.randn(b, fe, d, device=dev).to(torch.bfloat16)
    grad = torch.randn(b, d + p_pad, device=dev).to(torch.bfloat16)
    x_bytes = b * f * d * BF16
    fwd_bytes = x_bytes + b * (d + p_pad) * BF16
    # the backward reads the d direct and the P pair columns of each row
    bwd_bytes = b * (d + pairs) * BF16 + 2 * x_bytes

    runs = []
    for variant, name in VARIANTS:
        runs.append({"name": f"interact_cat_fwd {name}", "bytes": fwd_bytes,
                     "step": lambda v=variant: ext.interact_cat_fwd(
                         bot, emb, p_pad, v)})
        runs.append({"name": f"interact_cat_bwd {name}", "bytes": bwd_bytes,
                     "step": lambda v=variant: ext.interact_cat_bwd(
                         grad, bot, emb, v)})
    for run in runs:
        run["us"] = []
        for _ in range(args.warmup):
            run["step"]()
    torch.cuda.synchronize()
    for _ in range(args.loops):
        for run in runs:
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                run["step"]()
            e.record()
            torch.cuda.synchronize()
            run["us"].append(s.elapsed_time(e) * 1e3 / args.iters)

    print(f"B={b} Fe={fe} D={d} P_pad={p_pad}: us per call, median of "
          f"{args.loops} loops x {args.iters} calls (spread), MB moved, "
          f"TB/s")
    for run in runs:
        v = run["us"]
        med = statistics.median(v)
        print(f"{run['name']:<26} {med:8.2f} ({max(v) - min(v):6.2f}) "
              f"{run['bytes'] / 1e6:7.2f} {run['bytes'] / med / 1e6:6.3f}",
              flush=True)


if __name__ == "__main__":
    main()
