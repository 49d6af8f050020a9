"""The MaskNet mask block h' = relu(LN((mask * h) W^T + b)) as one autograd
node on the gfx950 kernels of ops/hip/mask_kernels.hip.

Forward: one maskblock_fwd launch; the masked product is formed in
registers as the GEMM's A operand and the LayerNorm and the ReLU run on the
accumulators. Backward: ln_relu_bwd, the existing dW and dX kernels on
dz and the saved product p, then mask_split_bwd for dmask and dh.
docs/KERNELS.md ("mask_kernels.hip") has the numerical contract.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from deeprec_amd.ops.fused_mlp import _global_module_hooks, _has_hooks

MAX_WIDTH = 256     # out_features the forward kernel covers with one block


class _MaskBlock(torch.autograd.Function):
    """h, mask [M, K]; weight [N, K], bias [N] of the linear; gamma, beta
    [N] of the LayerNorm. Returns y [M, N] bf16. The fp32 master weight is
    cast to bf16 per call, as _FusedLinear does without a cache."""

    @staticmethod
    def forward(ctx, h, mask, weight, bias, gamma, beta, eps):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        h16 = h.to(torch.bfloat16).contiguous()
        m16 = mask.to(torch.bfloat16).contiguous()
        w16 = weight.detach().to(torch.bfloat16).contiguous()
        g32 = gamma.detach().float().contiguous()
        save = any(ctx.needs_input_grad)
        y, z, stats, p = ext.maskblock_fwd(
            m16, h16, w16, bias.detach().float().contiguous(), g32,
            beta.detach().float().contiguous(), eps, save)
        ctx.ext = ext
        ctx.dtypes = (h.dtype, mask.dtype)
        ctx.save_for_backward(h16, m16, w16, g32, y, z, stats, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = ctx.ext
        h16, m16, w16, g32, y, z, stats, p = ctx.saved_tensors
        dz, dgamma, dbeta = ext.ln_relu_bwd(
            dy.to(torch.bfloat16).contiguous(), y, z, stats, g32)
        dw, db = ext.linear_dw(dz, p, True)
        dh = dm = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dm, dh = ext.mask_split_bwd(ext.linear_dx(dz, w16), m16, h16)
            dh = dh.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
            dm = dm.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None
        return dh, dm, dw, db, dgamma, dbeta, None


def _fusable(h, mask, linear, norm) -> bool:
    rows = h.numel() // h.shape[-1] if h.shape[-1] else 0
    return (h.device.type == "cuda" and mask.device == h.device
            and rows > 0 and mask.shape == h.shape
            and type(linear) is nn.Linear and type(norm) is nn.LayerNorm
            and linear.bias is not None
            and 1 <= linear.out_features <= MAX_WIDTH
            and norm.elementwise_affine and norm.bias is not None
            and tuple(norm.normalized_shape) == (linear.out_features,)
            and not _global_module_hooks()
            and not _has_hooks(linear) and not _has_hooks(norm))


def mask_block(h: torch.Tensor, mask: torch.Tensor, linear: nn.Linear,
               norm: nn.LayerNorm) -> torch.Tensor:
    """relu(norm(linear(mask * h))) for h, mask [..., K]. On the GPU, for a
    plain nn.Linear with bias and out_features <= 256, an elementwise-affine
    nn.LayerNorm over the last axis and no module hooks, this is one
    autograd node on the mask-block kernels and the result is bf16. Anything
    else, the CPU included, is the torch formula in the input's dtype."""
    if _fusable(h, mask, linear, norm):
        lead = h.shape[:-1]
        y = _MaskBlock.apply(
            h.reshape(-1, h.shape[-1]), mask.reshape(-1, h.shape[-1]),
            linear.weight, linear.bias, norm.weight, norm.bias, norm.eps)
        return y.reshape(*lead, linear.out_features)
    x = mask * h
    if x.dtype == linear.weight.dtype:
        return torch.relu(norm(linear(x)))   # the modules: their hooks fire
    cast = lambda t: None if t is None else t.to(x.dtype)  # noqa: E731
    z = F.linear(x, cast(linear.weight), cast(linear.bias))
    return torch.relu(F.layer_norm(z, norm.normalized_shape,
                                   cast(norm.weight), cast(norm.bias),
                                   norm.eps))
