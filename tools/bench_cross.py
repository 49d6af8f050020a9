"""Microbenchmark of the DCNv2 cross stack alone.

Runs forward + backward of _CrossNet at B = 8192, L = 3 for
    D = 432, R = 32   (mlperf_dlrm_dcn)
    D = 429, full matrix (dcnv2)
with fused_train off (layer by layer in fp32 torch) and on (one autograd
node on the cross kernels).
Device events around each timed window; every configuration is warmed up
first; the timed loops visit the configurations in turn, so drift of the
machine lands on all of them alike. Reported: median over `--loops` loops
of the mean over `--iters` calls, and the spread (max - min) of the loops.
Eager only. Run on a GPU box:
    python -m tools.bench_cross
"""
import argparse
import statistics

import torch

from deeprec_amd.models.zoo import _CrossNet

SHAPES = [(432, 32), (429, 0)]      # (D, R)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--layers", type=int, default=3)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--loops", type=int, default=7)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_cross needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    b = args.batch
    runs = []
    for d, r in SHAPES:
        x0 = torch.randn(b, d, device=dev)
        gout = torch.randn(b, d, device=dev)
        plain = _CrossNet(d, args.layers, v2=True, low_rank=r).to(dev)
        for fused in (False, True):
            net = _CrossNet(d, args.layers, v2=True, low_rank=r,
                            fused_train=fused).to(dev)
            net.load_state_dict(plain.state_dict())

            def step(net=net, x0=x0, gout=gout):
                x = x0.detach().requires_grad_(True)
                net.zero_grad(set_to_none=True)
                net(x).backward(gout)
            runs.append({"name": f"stack fwd+bwd D={d} R={r} "
                                 f"fused_train={fused}", "step": step})
    for run in runs:
        run["ms"] = []
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
            run["ms"].append(s.elapsed_time(e) / args.iters)

    print(f"B={b} L={args.layers}: ms per call, median of {args.loops} "
          f"loops x {args.iters} calls (spread)")
    for run in runs:
        v = run["ms"]
        print(f"{run['name']:<48} {statistics.median(v):8.4f} "
              f"({max(v) - min(v):6.4f})", flush=True)


if __name__ == "__main__":
    main()
