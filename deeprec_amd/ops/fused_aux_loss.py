"""DIEN's auxiliary next-item loss as one autograd node.

For every sample b and step t < T - 1 with both steps valid, the click pair
[h_t | e_{t+1}] and the no-click pair [h_t | e_{perm[b], t+1}] go through the
two-layer aux net (sigmoid hidden layer, one logit) and a BCE against 1 and
0; the loss is the mean over the live pairs, 0 when there is none. GPU path:
ops/hip/dien_aux_kernels.hip, one MFMA kernel per direction that never
writes the concatenated rows, the hidden activations or the logits. Anything
the kernels do not take runs the torch composition with the same semantics.
"""
from __future__ import annotations

import torch
import torch.nn as nn

# what dien_aux_fwd / dien_aux_bwd take (dien_aux_kernels.hip)
DIEN_AUX_MAX_WIDTH, DIEN_AUX_MAX_HIDDEN = 64, 128


def dien_aux_workgroups(rows: int) -> int:
    """Workgroups the dien_aux kernels launch for `rows` = B (T - 1)
    flattened (sample, step) rows."""
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension().dien_aux_grid(rows)


class _DienAuxLoss(torch.autograd.Function):
    """Saves the inputs and the live-pair count only; backward recomputes
    the hidden activations and logits. Weights are used as bf16, biases as
    fp32. Nothing synchronises: the loss, the count and the upstream
    gradient stay on the device."""

    @staticmethod
    def forward(ctx, h, seq, mask_u8, perm, w1, b1, w2, b2):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        w1_16 = w1.detach().to(torch.bfloat16).contiguous()
        w2_16 = w2.detach().to(torch.bfloat16).reshape(-1).contiguous()
        b1f = b1.detach().float().contiguous()
        b2f = b2.detach().float().reshape(1)
        loss, msum = ext.dien_aux_fwd(h, seq, mask_u8, perm, w1_16, b1f,
                                      w2_16, b2f)
        ctx.ext = ext
        ctx.save_for_backward(msum, h, seq, mask_u8, perm, w1_16, b1f, w2_16,
                              b2f)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        dh, dclick, dnoclick, dw1, db1, dw2, db2 = ctx.ext.dien_aux_bwd(
            grad_out.float().contiguous(), *ctx.saved_tensors)
        return (dh, dclick.add_(dnoclick), None, None, dw1, db1,
                dw2.view(1, -1), db2)


def _composed(h_seq, seq, mask, perm, lin1, lin2):
    h = h_seq[:, :-1].float()
    click = seq[:, 1:].float()
    noclick = click[perm]
    m = mask[:, :-1].float() * mask[:, 1:].float()
    m = m * (perm != torch.arange(seq.shape[0], device=seq.device)) \
        .float().unsqueeze(1)

    def net(x):
        return lin2(torch.sigmoid(lin1(x))).squeeze(2)

    logit_c = net(torch.cat([h, click], -1))
    logit_n = net(torch.cat([h, noclick], -1))
    bce = nn.functional.binary_cross_entropy_with_logits
    lc = bce(logit_c, torch.ones_like(logit_c), reduction="none")
    ln = bce(logit_n, torch.zeros_like(logit_n), reduction="none")
    total, count = ((lc + ln) * m).sum(), m.sum()
    return torch.where(count > 0, total / count.clamp_min(1.0),
                       torch.zeros_like(total))


def dien_aux_loss(h_seq: torch.Tensor, seq: torch.Tensor, mask: torch.Tensor,
                  perm: torch.Tensor, lin1: nn.Linear,
                  lin2: nn.Linear) -> torch.Tensor:
    """h_seq [B,T,H] GRU states, seq [B,T,Di] item embeddings, mask [B,T]
    (nonzero = valid), perm [B] a permutation of the batch (the in-batch
    negatives; a sample paired with itself is dropped), lin1 = Linear(H + Di
    -> A) followed by a sigmoid, lin2 = Linear(A -> 1). Returns the scalar
    loss, never None: 0 when no pair is live. On the GPU, within the
    kernels' limits (H, Di % 4 == 0 in [4, 64], A % 16 == 0 in [16, 128],
    T >= 2, fp32 parameters), one fused node whose operands are rounded to
    bf16 once; anything else is the fp32 torch composition."""
    b, t, hd = h_seq.shape
    di, a = seq.shape[2], lin1.out_features
    if (h_seq.device.type == "cuda" and t >= 2
            and hd % 4 == 0 and 4 <= hd <= DIEN_AUX_MAX_WIDTH
            and di % 4 == 0 and 4 <= di <= DIEN_AUX_MAX_WIDTH
            and a % 16 == 0 and 16 <= a <= DIEN_AUX_MAX_HIDDEN
            and b * t * max(hd, di) < 2 ** 31
            and lin1.in_features == hd + di and lin2.in_features == a
            and lin2.out_features == 1
            and lin1.bias is not None and lin2.bias is not None
            and lin1.weight.dtype == torch.float32
            and lin2.weight.dtype == torch.float32):
        return _DienAuxLoss.apply(
            h_seq.float().contiguous(), seq.float().contiguous(),
            mask.ne(0).to(torch.uint8).contiguous(),
            perm.to(torch.int64).contiguous(), lin1.weight, lin1.bias,
            lin2.weight, lin2.bias)
    return _composed(h_seq, seq, mask, perm, lin1, lin2)
