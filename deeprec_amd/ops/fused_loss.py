"""Fused binary cross-entropy with logits, mean-reduced.

`bce_with_logits_mean(logits, labels)` is one HIP launch forward and one
backward (ops/hip/loss_kernels.hip) for what torch runs as about a dozen
elementwise and reduce launches. The forward sum has a fixed shape (a
strided sum per thread, then a block tree in one block), so the loss does
not depend on scheduling; the backward reads grad_out on the device, so
the pair is capture-safe. Soft labels are supported.

Everything the kernels do not cover goes to
torch.nn.functional.binary_cross_entropy_with_logits unchanged: weight,
pos_weight, a reduction other than "mean", CPU or non-fp32 or
non-contiguous or non-1-D inputs, labels that require grad, and B above
the extension's single-block cap (BCE_LOGITS_MEAN_MAX_B).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from deeprec_amd.ops.build_ext import require_extension


class _BceLogitsMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        ctx.save_for_backward(logits, labels)
        return require_extension().bce_logits_mean_fwd(logits, labels)

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels = ctx.saved_tensors
        return require_extension().bce_logits_mean_bwd(
            logits, labels, grad_out.contiguous()), None


def _fused_ok(logits, labels) -> bool:
    if logits.device.type != "cuda" or labels.device != logits.device:
        return False
    if logits.dtype != torch.float32 or labels.dtype != torch.float32:
        return False
    if logits.dim() != 1 or labels.shape != logits.shape:
        return False
    if not (logits.is_contiguous() and labels.is_contiguous()):
        return False
    if labels.requires_grad:
        return False
    return 1 <= logits.numel() <= require_extension().BCE_LOGITS_MEAN_MAX_B


def bce_with_logits_mean(logits: torch.Tensor, labels: torch.Tensor,
                         weight=None, pos_weight=None,
                         reduction: str = "mean") -> torch.Tensor:
    if (weight is None and pos_weight is None and reduction == "mean"
            and _fused_ok(logits, labels)):
        return _BceLogitsMean.apply(logits, labels)
    return F.binary_cross_entropy_with_logits(
        logits, labels, weight=weight, pos_weight=pos_weight,
        reduction=reduction)
