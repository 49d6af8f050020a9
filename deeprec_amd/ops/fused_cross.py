"""DCNv2 cross stacks on the gfx950 kernels of ops/hip/cross_kernels.hip.

x_{l+1} = x0 * u_l + x_l with u_l = W_l x_l + b_l, or, low rank,
u_l = U_l (V_l x_l) + b_l. The residual stream and its gradient stay fp32,
the GEMMs run in bf16 on the MFMA with fp32 accumulation and the cross
update is their epilogue; docs/KERNELS.md ("cross_kernels.hip") states every
rounding of both directions.

cross_net is the full-matrix inference path and records no gradient.
cross_stack is one autograd node for a whole stack of full-matrix and
low-rank layers, eager only: it has not been run under graph capture.

The weights are cast to bf16 on every call: there is no weight cache for
these layers.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

MAX_RANK = 128      # k_cross_lr_bwd keeps a wave's [16, R] in LDS


def cross_net(x0: torch.Tensor,
              layers: Sequence[Tuple[torch.Tensor, torch.Tensor]]
              ) -> torch.Tensor:
    """Run a full-matrix DCNv2 cross stack on x0 (fp32 [B, D] on the GPU)
    and return x_L in fp32. layers: per layer (W [D, D], b [D]) on x0's
    device. No gradient is recorded, so a call that would need one (grad
    mode on and x0 or a parameter requiring grad) is an error."""
    if x0.device.type != "cuda" or x0.dtype != torch.float32 or x0.dim() != 2:
        raise ValueError("cross_net: x0 must be an fp32 [B, D] GPU matrix")
    if not layers or any(len(layer) != 2 for layer in layers):
        raise ValueError("cross_net: layers must be a non-empty sequence of "
                         "(W, b)")
    params = [p for layer in layers for p in layer]
    if any(p.device != x0.device for p in params):
        raise ValueError("cross_net: every W and b must be on x0's device "
                         f"{x0.device}")
    if torch.is_grad_enabled() and (
            x0.requires_grad or any(p.requires_grad for p in params)):
        raise RuntimeError("cross_net is forward only: call it under "
                           "torch.no_grad(), or with inputs that need no "
                           "gradient")
    from deeprec_amd.ops.build_ext import require_extension
    ext = require_extension()
    with torch.no_grad():
        x0 = x0.contiguous()
        x, a16 = x0, x0.to(torch.bfloat16)
        for w, b in layers:
            x, a16, _ = ext.cross_fwd(a16, w.to(torch.bfloat16).contiguous(),
                                      b.float().contiguous(), x0, x, False)
    return x


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.bfloat16).contiguous()


def _bf16_t(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.bfloat16).t().contiguous()


class _CrossStack(torch.autograd.Function):
    """The whole stack as one node. kinds[l] is the number of weights of
    layer l (1: W; 2: V, U); params holds each layer's weights and then its
    bias. Saved per layer: a_l = bf(x_l), bf(u_l) and, low rank, t_l."""

    @staticmethod
    def forward(ctx, x0, kinds, *params):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        save = any(ctx.needs_input_grad)
        x0 = x0.detach().contiguous()
        x, a16 = x0, x0.to(torch.bfloat16)
        saved, it = [x0], iter(params)
        for kind in kinds:
            if kind == 1:
                w, b = next(it), next(it)
                xn, an16, u16 = ext.cross_fwd(
                    a16, _bf16(w), b.detach().float().contiguous(), x0, x,
                    save)
                saved += [a16, u16]
            else:
                v, u, b = next(it), next(it), next(it)
                t16 = ext.linear_fwd(a16, _bf16(v), torch.Tensor(), 0)
                xn, an16, u16 = ext.cross_fwd(
                    t16, _bf16(u), b.detach().float().contiguous(), x0, x,
                    save)
                saved += [a16, u16, t16]
            x, a16 = xn, an16
        if save:
            ctx.kinds = kinds
            ctx.save_for_backward(*saved, *params)
        return x

    @staticmethod
    def backward(ctx, gout):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        kinds = ctx.kinds
        n_saved = 1 + sum(k + 1 for k in kinds)
        saved = ctx.saved_tensors[:n_saved]
        params = ctx.saved_tensors[n_saved:]
        x0 = saved[0]
        g = gout.float().contiguous()
        dx0 = torch.empty_like(x0)
        ext.zero_f32(dx0.view(-1))
        grads = [None] * len(params)
        s_end, p_end = n_saved, len(params)
        for kind in reversed(kinds):
            s_end, p_end = s_end - (kind + 1), p_end - (kind + 1)
            a16, u16 = saved[s_end], saved[s_end + 1]
            if kind == 1:
                du16 = ext.cross_du(g, x0, u16, dx0)
                dw, db = ext.linear_dw(du16, a16, True)
                g = ext.cross_dx(du16, _bf16_t(params[p_end]), g)
                grads[p_end:p_end + 2] = [dw, db]
            else:
                t16 = saved[s_end + 2]
                v, u = params[p_end], params[p_end + 1]
                g, du16, dt16 = ext.cross_lr_bwd(g, x0, u16, _bf16_t(u),
                                                 _bf16_t(v), dx0)
                du_w, db = ext.linear_dw(du16, t16, True)
                dv, _ = ext.linear_dw(dt16, a16, False)
                grads[p_end:p_end + 3] = [dv, du_w, db]
        grads = [gr.to(p.dtype) for gr, p in zip(grads, params)]
        return (dx0 + g, None, *grads)


def cross_stack(x0: torch.Tensor, layers: Sequence[Tuple[torch.Tensor, ...]]
                ) -> torch.Tensor:
    """Run a DCNv2 cross stack on x0 (fp32 [B, D] on the GPU) and return
    x_L in fp32, as one autograd node. layers: per layer (W [D, D], b [D])
    or, low rank, (V [R, D], U [D, R], b [D]) with 1 <= R <= 128, all on
    x0's device. Without a recorded gradient the same forward kernels run
    and nothing is saved."""
    if x0.device.type != "cuda" or x0.dtype != torch.float32 or x0.dim() != 2:
        raise ValueError("cross_stack: x0 must be an fp32 [B, D] GPU matrix")
    if not layers or any(len(layer) not in (2, 3) for layer in layers):
        raise ValueError("cross_stack: layers must be a non-empty sequence "
                         "of (W, b) or (V, U, b)")
    params = [p for layer in layers for p in layer]
    if any(p.device != x0.device for p in params):
        raise ValueError("cross_stack: every weight and bias must be on "
                         f"x0's device {x0.device}")
    for layer in layers:
        if len(layer) == 3 and not 1 <= layer[0].shape[0] <= MAX_RANK:
            raise ValueError("cross_stack: the rank must be in [1, "
                             f"{MAX_RANK}], got {layer[0].shape[0]}")
    kinds = tuple(len(layer) - 1 for layer in layers)
    return _CrossStack.apply(x0, kinds, *params)
