"""DCNv2 full-matrix cross stack, forward only, on the gfx950 kernel of
ops/hip/cross_kernels.hip.

x_{l+1} = x0 * u_l + x_l with u_l = W_l x_l + b_l. The residual stream stays
fp32, the GEMM runs in bf16 on the MFMA with fp32 accumulation and the cross
update is its epilogue; docs/KERNELS.md ("cross_kernels.hip") states every
rounding. There is no autograd node: this is the inference path, training
keeps the layer-by-layer fp32 path.

The weights are cast to bf16 on every call: there is no weight cache for
these layers.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch


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
