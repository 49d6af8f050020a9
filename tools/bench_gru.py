"""Microbenchmark of the GRU / AUGRU recurrence kernels inside FusedGRU.

Runs forward + backward of FusedGRU alone at B = 16384, T = 50 (the DIEN
benchmark shape) for
    impl="wave" and impl="tile" at H = 32,
    impl="tile" at H = 36 and 64,
each as plain GRU and as AUGRU, and prints per-kernel times: device events
around the two recurrence calls (gru_fwd / gru_bwd or gru_tile_fwd /
gru_tile_bwd), not around the whole module, whose time (GEMMs, casts and
the h_prev shift included) is listed next to them. Every configuration is
warmed up first; the timed loops visit the configurations in turn, so
drift of the machine lands on all of them alike. Reported: median over
`--loops` loops of the mean over `--iters` steps, and the spread (max -
min) of the loops. Run on a GPU box:
    python -m tools.bench_gru
"""
import argparse
import statistics

import torch

from deeprec_amd.ops import build_ext
from deeprec_amd.ops.fused_gru import FusedGRU

CONFIGS = [("wave", 32), ("tile", 32), ("tile", 36), ("tile", 64)]
KERNELS = {"gru_fwd": "fwd", "gru_tile_fwd": "fwd",
           "gru_bwd": "bwd", "gru_tile_bwd": "bwd"}


class TimedExt:
    """The extension with device events around the recurrence calls."""

    def __init__(self, ext):
        self._ext = ext
        self.spans = {"fwd": [], "bwd": []}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        kind = KERNELS.get(name)
        if kind is None:
            return fn

        def timed(*args):
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*args)
            e.record()
            self.spans[kind].append((s, e))
            return out
        return timed

    def take(self):
        """Mean ms per call of the spans recorded since the last take()."""
        out = {k: sum(s.elapsed_time(e) for s, e in v) / max(len(v), 1)
               for k, v in self.spans.items()}
        self.spans = {"fwd": [], "bwd": []}
        return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16384)
    p.add_argument("--seq_len", type=int, default=50)
    p.add_argument("--input_size", type=int, default=32)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--loops", type=int, default=5)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_gru needs a GPU"
    dev = torch.device("cuda", 0)
    timed = TimedExt(build_ext.require_extension())
    build_ext.require_extension = lambda: timed

    torch.manual_seed(0)
    b, t = args.batch, args.seq_len
    x = torch.randn(b, t, args.input_size, device=dev)
    alpha = torch.rand(b, t, device=dev)
    runs = []
    for impl, h in CONFIGS:
        gru = FusedGRU(args.input_size, h, impl=impl).to(dev)
        dh = torch.randn(b, t, h, device=dev)
        for augru in (False, True):
            runs.append({"impl": impl, "h": h, "augru": augru, "gru": gru,
                         "dh": dh, "fwd": [], "bwd": [], "module": []})

    def step(r):
        xi = x.detach().requires_grad_(True)
        ai = alpha.detach().requires_grad_(True) if r["augru"] else None
        r["gru"](xi, ai).backward(r["dh"])

    for r in runs:
        for _ in range(args.warmup):
            step(r)
    torch.cuda.synchronize()
    timed.take()
    for _ in range(args.loops):
        for r in runs:
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                step(r)
            e.record()
            torch.cuda.synchronize()
            k = timed.take()
            r["fwd"].append(k["fwd"])
            r["bwd"].append(k["bwd"])
            r["module"].append(s.elapsed_time(e) / args.iters)

    def cell(v):
        return f"{statistics.median(v):8.3f} ({max(v) - min(v):5.3f})"

    print(f"B={b} T={t} D={args.input_size}: ms per call, median of "
          f"{args.loops} loops x {args.iters} steps (spread)")
    print(f"{'impl':>5} {'H':>3} {'cell':>6} | {'recurrence fwd':>16} "
          f"{'recurrence bwd':>16} {'module fwd+bwd':>16}")
    for r in runs:
        print(f"{r['impl']:>5} {r['h']:>3} "
              f"{'AUGRU' if r['augru'] else 'GRU':>6} | {cell(r['fwd']):>16} "
              f"{cell(r['bwd']):>16} {cell(r['module']):>16}")


if __name__ == "__main__":
    main()
