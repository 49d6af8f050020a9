"""Grouped experts and the gate mixture of MMoE / PLE as one autograd node
on the gfx950 kernels of ops/hip/moe_kernels.hip.

expert_mixture(x, experts, gate_logits, mask) runs E FusedMLP experts of
identical layer shapes over one input and mixes them per task:

    mix[t] = sum_e softmax_e(gate_logits[:, t, e] | mask[t, e]) * expert_e(x)

Forward: one expert_fwd launch per hidden layer (the expert is grid z) and
one expert_mix_fwd for the last layer, the softmax and the mixture.
Backward: expert_mix_bwd, per expert the existing dW kernel on the expert's
contiguous slab, expert_dx between layers and, where x wants a gradient,
expert_dx(reduce=True), which sums the experts' input gradients in one
accumulator. All stacked tensors are expert-major: [E, B, .] activations,
[E, N, K] weights, [T, B, H] the mixture. docs/KERNELS.md
("moe_kernels.hip") has the numerical contract.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from deeprec_amd.ops.fused_mlp import (_ACT_ID, FusedLinear, FusedMLP,
                                       _global_module_hooks, _has_hooks)

MAX_EXPERTS = 16
MAX_TASKS = 4


class _ExpertMixture(torch.autograd.Function):
    """meta: (mask [T,E] uint8 host tensor, acts per layer, and per expert
    and layer the (w16_cache, dw_ws) pair); params: for each expert, for
    each layer, weight and bias. Returns mix [T, B, H] bf16."""

    @staticmethod
    def forward(ctx, x, gate_logits, meta, *params):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        mask, acts, slots = meta
        n_exp, n_lay = len(slots), len(acts)
        x16 = x.to(torch.bfloat16).contiguous()
        gl = gate_logits.float().contiguous()
        w16s, biases = [], []
        for i in range(n_lay):
            ws = []
            for e in range(n_exp):
                cache = slots[e][i][0]
                ws.append(cache if cache is not None
                          else params[2 * (e * n_lay + i)].detach())
            w16s.append(torch.stack(ws).to(torch.bfloat16))
            biases.append(torch.stack(
                [params[2 * (e * n_lay + i) + 1].detach()
                 for e in range(n_exp)]).float())
        h, outs = x16, []
        for i in range(n_lay - 1):
            h = ext.expert_fwd(h, w16s[i], biases[i], acts[i])
            outs.append(h)
        save = any(ctx.needs_input_grad)
        mix, ex, p = ext.expert_mix_fwd(h, w16s[-1], biases[-1], acts[-1],
                                        gl, mask, save)
        ctx.ext, ctx.meta = ext, meta
        ctx.x_dtype, ctx.gate_dtype = x.dtype, gate_logits.dtype
        ctx.save_for_backward(x16, ex, p, *w16s, *outs)
        return mix

    @staticmethod
    def backward(ctx, dmix):
        ext = ctx.ext
        mask, acts, slots = ctx.meta
        n_exp, n_lay = len(slots), len(acts)
        x16, ex, p = ctx.saved_tensors[:3]
        w16s = ctx.saved_tensors[3:3 + n_lay]
        outs = ctx.saved_tensors[3 + n_lay:]
        g, dgate = ext.expert_mix_bwd(
            dmix.to(torch.bfloat16).contiguous(), p, ex, mask, acts[-1])
        grads = [None] * (2 * n_exp * n_lay)
        dx = None
        for i in range(n_lay - 1, -1, -1):
            for e in range(n_exp):
                xin = x16 if i == 0 else outs[i - 1][e]
                ws = slots[e][i][1]
                if ws is not None:
                    dw, db = ext.linear_dw_out(g[e], xin, ws, True)
                else:
                    dw, db = ext.linear_dw(g[e], xin, True)
                k = 2 * (e * n_lay + i)
                grads[k], grads[k + 1] = dw, db
            if i > 0:
                g = ext.expert_dx(g, w16s[i], outs[i - 1], acts[i - 1])
            elif ctx.needs_input_grad[0]:
                dx = ext.expert_dx(g, w16s[0], reduce=True).to(ctx.x_dtype)
        return (dx, dgate.to(ctx.gate_dtype), None, *grads)


def _fusable(x, experts, n_tasks) -> bool:
    """FusedMLP.forward's conditions for every expert, identical layer
    shapes and activations, and the kernels' limits on E and T."""
    rows = x.numel() // x.shape[-1] if x.shape[-1] else 0
    if (x.device.type != "cuda" or x.dim() != 2 or rows == 0
            or rows % 16 != 0 or _global_module_hooks()
            or not 1 <= len(experts) <= MAX_EXPERTS
            or not 1 <= n_tasks <= MAX_TASKS):
        return False
    for mlp in experts:
        if (type(mlp) is not FusedMLP or len(mlp) == 0 or _has_hooks(mlp)
                or any(type(m) is not FusedLinear or _has_hooks(m)
                       for m in mlp)):
            return False
    first = [(m.in_features, m.out_features, m.activation)
             for m in experts[0]]
    return all([(m.in_features, m.out_features, m.activation)
                for m in mlp] == first for mlp in experts[1:])


def expert_mixture(x: torch.Tensor, experts: Sequence[nn.Module],
                   gate_logits: torch.Tensor,
                   mask: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """x [B, K]; experts: E modules mapping [B, K] -> [B, H]; gate_logits
    [B, T, E]; mask [T, E] (nonzero: task t mixes expert e; default all).
    Returns T tensors [B, H]: per task the softmax of its logits over its
    experts times the experts' outputs. On the GPU, for FusedMLP experts of
    identical shapes, E <= 16 and T <= 4, this is one autograd node on the
    grouped kernels and the results are bf16; everything else (the
    conditions of FusedMLP.forward) takes the layer-by-layer torch path."""
    n_exp, n_tasks = len(experts), gate_logits.shape[1]
    if mask is None:
        mask = torch.ones(n_tasks, n_exp, dtype=torch.uint8)
    mask = mask.to("cpu", torch.uint8).contiguous()
    if tuple(mask.shape) != (n_tasks, n_exp) or gate_logits.shape[2] != n_exp:
        raise ValueError(
            f"gate_logits is {tuple(gate_logits.shape)} and mask "
            f"{tuple(mask.shape)} for {n_exp} experts")
    if not bool(mask.any(1).all()):
        raise ValueError("a task mixes no expert")
    if _fusable(x, experts, n_tasks):
        acts = tuple(_ACT_ID[m.activation] for m in experts[0])
        slots = tuple(tuple((m.w16_cache, m.dw_ws) for m in mlp)
                      for mlp in experts)
        params = [q for mlp in experts for m in mlp
                  for q in (m.weight, m.bias)]
        mix = _ExpertMixture.apply(x, gate_logits, (mask, acts, slots),
                                   *params)
        return list(mix.unbind(0))
    ex = torch.stack([e(x) for e in experts], 1).float()   # [B, E, H]
    out = []
    for t in range(n_tasks):
        idx = mask[t].nonzero().flatten().tolist()
        g = torch.softmax(gate_logits[:, t, idx], dim=1)
        sel = ex if len(idx) == n_exp else ex[:, idx]
        out.append(torch.einsum("be,beh->bh", g, sel))
    return out
