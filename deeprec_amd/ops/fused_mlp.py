"""FusedMLP — bf16 MFMA linear layers with fp32 master weights.

GPU path uses the hand-written gfx950 kernels (ops/hip/dense_kernels.hip);
CPU path falls back to torch (the numerics reference). This mirrors the
reference's keep_weights bf16 scope (fp32 master weights, bf16 compute —
reference: python/ops/variable_scope.py:3008) with the cast fused into the
layer instead of graph-level cast nodes.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

_ACT_ID = {None: 0, "none": 0, "relu": 1, "sigmoid": 2}


class _FusedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act_id, w16_cache=None, dw_ws=None):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        # w16_cache: bf16 shadow refreshed once per optimizer step by
        # enable_weight_cache() — replaces a per-layer cast kernel
        w16 = (w16_cache if w16_cache is not None
               else weight.detach().to(torch.bfloat16).contiguous())
        x16 = x.to(torch.bfloat16).contiguous()
        out = ext.linear_fwd(x16, w16, bias.detach().float(), act_id)
        ctx.ext = ext
        ctx.act_id = act_id
        ctx.x_dtype = x.dtype
        ctx.dw_ws = dw_ws
        ctx.save_for_backward(x16, w16, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x16, w16, out = ctx.saved_tensors
        ext = ctx.ext
        g = grad_out.to(torch.bfloat16).contiguous()
        if ctx.act_id != 0:
            g = ext.act_bwd(g, out, ctx.act_id)
        # an input that needs no gradient (the model's dense features)
        # costs neither the dX GEMM nor the cast back
        dx = (ext.linear_dx(g, w16).to(ctx.x_dtype)
              if ctx.needs_input_grad[0] else None)
        # direct col-fragment dW: measured faster end-to-end than the
        # transpose-then-row-load variant (torch .t().contiguous() costs
        # ~12us/copy, more than the strided-fragment penalty it removes)
        if ctx.dw_ws is not None:
            # FlatDenseAdam mode: dW/db land in the optimizer's flat
            # gradient buffer (zero-filled + accumulated by the kernel)
            dw, db = ext.linear_dw_out(g, x16, ctx.dw_ws, True)
        else:
            dw, db = ext.linear_dw(g, x16, True)
        return dx, dw, db, None, None, None


def _adjacent_span(slices: Sequence[torch.Tensor]) -> Optional[torch.Tensor]:
    """One 1-D view over the union of `slices` if they are contiguous fp32
    slices of one storage lying back to back (in any order), else None."""
    first = slices[0]
    base = first.untyped_storage().data_ptr()
    for ws in slices:
        if (ws.dtype != torch.float32 or ws.dim() != 1
                or not ws.is_contiguous()
                or ws.untyped_storage().data_ptr() != base):
            return None
    order = sorted(slices, key=lambda t: t.data_ptr())
    for a, b in zip(order, order[1:]):
        if a.data_ptr() + 4 * a.numel() != b.data_ptr():
            return None
    total = sum(ws.numel() for ws in slices)
    return torch.as_strided(order[0], (total,), (1,),
                            order[0].storage_offset())


# linear_dx takes the LDS-staged kernel from this GEMM-K (= layer width N)
# up. There the epilogue's prev_out loads cost more than the k_act_bwd they
# replace (8192x256->512: 13.3 -> 19.7 us against 5.7 us; the direct kernel
# pays 2-3 us against 5 us — profiles/PERF_LOG.md), so such layers keep the
# unfused pair.
_DX_FUSE_BELOW_N = 128


class _FusedMLPChain(torch.autograd.Function):
    """A whole FusedLinear stack as ONE autograd node. Forward makes the
    per-layer linear_fwd calls; backward hands each layer's activation
    gradient to the dX kernel of the layer above it (epilogue-fused, no
    k_act_bwd pass) where that is the cheaper form, clears a tower's adjacent flat-gradient slices with
    one fill, and skips dX of the first layer when the input needs no
    gradient. Results are bit-identical to the per-layer path.
    meta: per layer (act_id, w16_cache, dw_ws); params: w0, b0, w1, b1, …"""

    @staticmethod
    def forward(ctx, x, meta, *params):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        x16 = x.to(torch.bfloat16).contiguous()
        h = x16
        w16s, outs = [], []
        for i, (act_id, w16_cache, _) in enumerate(meta):
            weight, bias = params[2 * i], params[2 * i + 1]
            w16 = (w16_cache if w16_cache is not None
                   else weight.detach().to(torch.bfloat16).contiguous())
            h = ext.linear_fwd(h, w16, bias.detach().float(), act_id)
            w16s.append(w16)
            outs.append(h)
        ctx.ext = ext
        ctx.acts = [m[0] for m in meta]
        ctx.wss = [m[2] for m in meta]
        ctx.x_dtype = x.dtype
        ctx.save_for_backward(x16, *w16s, *outs)
        return h

    @staticmethod
    def backward(ctx, grad_out):
        ext, acts, wss = ctx.ext, ctx.acts, ctx.wss
        n = len(acts)
        saved = ctx.saved_tensors
        x16, w16s, outs = saved[0], saved[1:1 + n], saved[1 + n:]
        g = grad_out.to(torch.bfloat16).contiguous()
        if acts[-1] != 0:
            g = ext.act_bwd(g, outs[-1], acts[-1])
        # flat-Adam mode: the tower's [dW | db] slices lie back to back in
        # the optimizer's gradient buffer -> one fill instead of one per
        # layer; anything else keeps the per-layer zero-then-accumulate
        one_fill = False
        if all(ws is not None for ws in wss):
            span = _adjacent_span(wss)
            if span is not None:
                ext.zero_f32(span)
                one_fill = True
        grads = [None] * (2 * n)
        dx = None
        for i in range(n - 1, -1, -1):
            xin = x16 if i == 0 else outs[i - 1]
            if wss[i] is not None:
                dw, db = ext.linear_dw_out(g, xin, wss[i], True,
                                           zero=not one_fill)
            else:
                dw, db = ext.linear_dw(g, xin, True)
            grads[2 * i], grads[2 * i + 1] = dw, db
            if i > 0 and (acts[i - 1] == 0
                          or g.shape[1] < _DX_FUSE_BELOW_N):
                g = ext.linear_dx(g, w16s[i], outs[i - 1], acts[i - 1])
            elif i > 0:
                g = ext.act_bwd(ext.linear_dx(g, w16s[i]), outs[i - 1],
                                acts[i - 1])
            elif ctx.needs_input_grad[0]:
                dx = ext.linear_dx(g, w16s[0]).to(ctx.x_dtype)
        return (dx, None, *grads)


class FusedLinear(nn.Module):
    """Linear(+activation) with fp32 master weight, bf16 MFMA compute on
    GPU. activation: None | 'relu' | 'sigmoid'. 3D inputs are flattened
    over the leading dims."""

    def __init__(self, in_features: int, out_features: int,
                 relu: bool = True, activation: Optional[str] = "unset"):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.activation = ("relu" if relu else None) \
            if activation == "unset" else activation
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.zeros(out_features))
        # torch Linear default init (kaiming uniform)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_features)
        nn.init.uniform_(self.bias, -bound, bound)
        self.w16_cache = None  # set by enable_weight_cache()
        self.dw_ws = None      # set by FlatDenseAdam (flat grad slice)

    def forward(self, x):
        lead = x.shape[:-1]
        flat = x.reshape(-1, x.shape[-1])
        if x.device.type == "cuda" and flat.shape[0] % 16 == 0:
            out = _FusedLinear.apply(flat, self.weight, self.bias,
                                     _ACT_ID[self.activation],
                                     self.w16_cache, self.dw_ws)
        else:
            out = nn.functional.linear(flat, self.weight.to(flat.dtype),
                                       self.bias.to(flat.dtype))
            if self.activation == "relu":
                out = nn.functional.relu(out)
            elif self.activation == "sigmoid":
                out = torch.sigmoid(out)
        return out.reshape(*lead, self.out_features)


class _DotInteraction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, p_pad):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        f16 = feats.to(torch.bfloat16).contiguous()
        out = ext.interact_fwd(f16, p_pad)
        ctx.ext = ext
        ctx.f_dtype = feats.dtype
        ctx.save_for_backward(f16)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (f16,) = ctx.saved_tensors
        df = ctx.ext.interact_bwd(grad_out.to(torch.bfloat16), f16)
        return df.to(ctx.f_dtype), None


def dot_interaction(feats: torch.Tensor, p_pad: int = None) -> torch.Tensor:
    """feats [B, F, D] -> pairwise dots [B, p_pad] (i<j upper triangle,
    zero-padded). Fused gfx950 kernel on GPU; torch fallback elsewhere."""
    b, f, d = feats.shape
    p = f * (f - 1) // 2
    p_pad = p_pad or p
    if feats.device.type == "cuda" and (f * d) % 8 == 0:
        return _DotInteraction.apply(feats, p_pad)
    z = torch.bmm(feats.float(), feats.float().transpose(1, 2))
    iu = torch.triu_indices(f, f, offset=1, device=feats.device)
    out = z[:, iu[0], iu[1]]
    if p_pad > p:
        out = torch.nn.functional.pad(out, (0, p_pad - p))
    return out.to(feats.dtype)


class _DotInteractionCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bot, emb, p_pad):
        from deeprec_amd.ops.build_ext import require_extension
        ext = require_extension()
        b16 = bot.to(torch.bfloat16).contiguous()
        e16 = emb.to(torch.bfloat16).contiguous()
        out = ext.interact_cat_fwd(b16, e16, p_pad)
        ctx.ext = ext
        ctx.dtypes = (bot.dtype, emb.dtype)
        ctx.save_for_backward(b16, e16)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        b16, e16 = ctx.saved_tensors
        dbot, demb = ctx.ext.interact_cat_bwd(
            grad_out.to(torch.bfloat16), b16, e16)
        bd, ed = ctx.dtypes
        return dbot.to(bd), demb.to(ed), None


def dot_interaction_cat(bot: torch.Tensor, emb: torch.Tensor,
                        p_pad: int) -> torch.Tensor:
    """bot [B,D] + emb [B,F,D] -> [B, D + p_pad] = [bot | pairwise dots
    over [bot; emb] rows, i<j upper triangle, zero-padded] in ONE fused
    kernel per direction — removes the feats-assembly cat AND the
    top-MLP input cat. Torch fallback composes the same math."""
    if bot.device.type == "cuda" and bot.shape[1] % 8 == 0:
        out = _DotInteractionCat.apply(bot, emb, p_pad)
        # keep the caller's compute dtype (the fp32 debug path feeds
        # plain nn.Linear layers)
        return out if out.dtype == bot.dtype else out.to(bot.dtype)
    feats = torch.cat([bot.unsqueeze(1), emb.to(bot.dtype)], dim=1)
    return torch.cat([bot, dot_interaction(feats, p_pad)], dim=1)


def _has_hooks(m: nn.Module) -> bool:
    return bool(m._forward_hooks or m._forward_pre_hooks
                or m._backward_hooks or m._backward_pre_hooks)


def _global_module_hooks() -> bool:
    """Hooks registered for every nn.Module (register_module_forward_hook
    and its kin) must fire per layer like a layer's own hooks."""
    g = torch.nn.modules.module
    return bool(g._global_forward_hooks or g._global_forward_pre_hooks
                or g._global_backward_hooks or g._global_backward_pre_hooks)


class FusedMLP(nn.Sequential):
    """nn.Sequential of FusedLinear layers (same state_dict keys, indexing,
    slicing and iteration) whose GPU forward runs the stack as one
    _FusedMLPChain node. Falls back to layer-by-layer nn.Sequential.forward
    off the GPU, for row counts the kernels do not take, when a layer
    carries hooks or module-global hooks are registered (they must fire
    per layer), or when a member is not a FusedLinear."""

    def forward(self, x):
        layers = list(self)
        rows = x.numel() // x.shape[-1] if x.shape[-1] else 0
        if (not layers or x.device.type != "cuda" or rows == 0
                or rows % 16 != 0 or _global_module_hooks()
                or any(type(m) is not FusedLinear or _has_hooks(m)
                       for m in layers)):
            return super().forward(x)
        lead = x.shape[:-1]
        flat = x.reshape(-1, x.shape[-1])
        meta = tuple((_ACT_ID[m.activation], m.w16_cache, m.dw_ws)
                     for m in layers)
        params = [p for m in layers for p in (m.weight, m.bias)]
        out = _FusedMLPChain.apply(flat, meta, *params)
        return out.reshape(*lead, layers[-1].out_features)


def fused_mlp(sizes: List[int], in_dim: int,
              final_activation: bool = True) -> FusedMLP:
    layers = []
    d = in_dim
    for i, h in enumerate(sizes):
        layers.append(FusedLinear(d, h,
                                  relu=final_activation or i + 1 < len(sizes)))
        d = h
    return FusedMLP(*layers)


def prep_dense(x: torch.Tensor, k_pad: int, fused: bool = True):
    """Zero-pad x [M,K] to k_pad columns. Where a FusedMLP will take the
    result through its kernels (fused, fp32 GPU matrix, rows % 16 == 0, no
    gradient wanted) the pad and the layer's fp32 -> bf16 cast are ONE
    kernel and the result is bf16; every other input is padded by torch
    and keeps its dtype."""
    if (fused and x.device.type == "cuda" and x.dtype == torch.float32
            and x.dim() == 2 and 0 < x.shape[1] < k_pad
            and x.shape[0] > 0 and x.shape[0] % 16 == 0
            and not x.requires_grad):
        from deeprec_amd.ops.build_ext import require_extension
        return require_extension().pad_cast_bf16(x.contiguous(), k_pad)
    if x.shape[-1] < k_pad:
        x = nn.functional.pad(x, (0, k_pad - x.shape[-1]))
    return x


def enable_weight_cache(model: nn.Module):
    """Give every FusedLinear a bf16 weight shadow and return a refresh()
    callable (ONE multi-tensor cast) to run after each optimizer step —
    set it as the optimizer's post_step_hook. Replaces the per-layer
    fp32->bf16 cast kernels (~4.6 us each) in the hot loop. Call refresh()
    manually after any out-of-band weight mutation (checkpoint restore,
    broadcast)."""
    mods = [m for m in model.modules() if isinstance(m, FusedLinear)]
    if not mods:
        return None
    shadows, masters = [], []
    for m in mods:
        m.w16_cache = m.weight.detach().to(torch.bfloat16).contiguous()
        shadows.append(m.w16_cache)
        masters.append(m.weight.detach())

    def refresh():
        torch._foreach_copy_(shadows, masters)

    return refresh
