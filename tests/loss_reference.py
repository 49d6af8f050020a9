"""fp64 reference and error bounds for the fused BCE-with-logits (mean)
kernels in ops/hip/loss_kernels.hip. No GPU needed.

Notation: u = 2^-24, the unit roundoff of fp32 (half an ulp, relative).

Forward bound
-------------
The kernel evaluates, in fp32,
    l = (max(x,0) - x*y) + log1p(exp(-|x|))
with 0 <= y <= 1.
  * max(x,0) is exact. x*y and the subtraction round once each (or once
    together as an fma): at most 2u|x|.
  * exp is within 1 ulp (relative 2u) and its argument is exact; log1p
    turns a relative error d of its argument e into at most d*e/(1+e)
    <= d/2, so u; log1p itself is within 2 ulp of a value <= ln 2, so
    4u*0.7 < 3u. Together under 4u.
  * the final addition rounds to u*l <= u(|x| + 1).
So each term is within 6u(|x| + 1) =: TERM_C * u * (|x| + 1) of its exact
value, and the mean of the terms within the mean of that.

The reduction: thread t adds the terms t, t+1024, ... serially
(ceil(B/1024) additions counting the one onto 0), the block folds 1024
partials in a binary tree (10 levels), and the total is divided by B (one
more rounding). Every term is >= 0, so every partial sum is <= the total S
and each of the `depth` roundings on a term's path to the result is at
most u*S (first order): depth * u * S / B = depth * u * mean(l).

    bound = mean(TERM_C*u*(|x|+1)) + depth*u*mean(l),
    depth = ceil(B/1024) + 10 + 1.

Backward bound
--------------
The kernel evaluates g = num/(1+e) * (grad_out/B), e = exp(-|x|),
    num = (1-y) - y*e   for x >= 0,     num = e*(1-y) - y   for x < 0,
which is (sigmoid(x) - y)(1+e) exactly.
  * Absolute part. 1-y is exact for y >= 1/2 (Sterbenz) and within u/2
    otherwise. The error of e (relative 2u) enters num as 2u*y*e (x >= 0)
    or 2u*(1-y)*e (x < 0). After the division by 1+e these are at most
    u/2 and 2u*e/(1+e)*max(y, 1-y). Where sigmoid(x) is close to y (the
    only place an absolute term matters) x >= 0 has y >= 1/2, so 1-y is
    exact, and e/(1+e) <= 1/2 throughout: what does not scale with the
    result stays below u. Away from cancellation the same quantities are
    a small multiple of u*|sigmoid(x) - y| and go to the relative part.
  * Relative part. The fma, 1+e, the division, grad_out/B and the final
    product round once each: 5u, plus at most 2u from the paragraph above,
    plus second-order terms: BWD_REL_C = 8.

    bound = BWD_REL_C*u*|ref| + u*|grad_out|/B.
"""
import math

import torch

U = 2.0 ** -24
LOSS_BLOCK = 1024      # kLossBlock in loss_kernels.hip
TERM_C = 6.0
BWD_REL_C = 8.0
FIXED_POINTS = (0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0)


def make_inputs(b, labels, seed):
    """fp32 (logits, labels) on the CPU: randn*4 logits with the fixed
    points written over the first positions (as many as fit)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(b, generator=gen) * 4
    k = min(b, len(FIXED_POINTS))
    x[:k] = torch.tensor(FIXED_POINTS[:k])
    if labels == "hard":
        y = (torch.rand(b, generator=gen) < 0.3).float()
    else:
        y = torch.rand(b, generator=gen)
    return x, y


def ref_terms(x, y):
    x, y = x.double(), y.double()
    return x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))


def ref_loss(x, y):
    return float(ref_terms(x, y).mean())


def reduction_depth(b):
    return math.ceil(b / LOSS_BLOCK) + int(math.log2(LOSS_BLOCK)) + 1


def fwd_bound(x, y):
    per_term = float((TERM_C * U * (x.double().abs() + 1)).mean())
    return per_term + reduction_depth(x.numel()) * U * ref_loss(x, y)


def ref_grad(x, y, grad_out):
    """(sigmoid(x) - y) * grad_out / B in fp64, over the common denominator
    so that fp64 itself does not cancel sigmoid(88) against 1."""
    x, y = x.double(), y.double()
    e = torch.exp(-x.abs())
    num = torch.where(x >= 0, (1 - y) - y * e, e * (1 - y) - y)
    return num / (1 + e) * (float(grad_out) / x.numel())


def bwd_bound(ref, grad_out, b):
    return BWD_REL_C * U * ref.abs() + U * abs(float(grad_out)) / b


def emulate_fwd_fp32(x, y):
    """The kernel's forward in fp32 on the CPU, in its summation order."""
    b = x.numel()
    l32 = ((x.clamp(min=0) - x * y)
           + torch.log1p(torch.exp(-x.abs()))).float()
    pad = (-b) % LOSS_BLOCK
    grid = torch.cat([l32, torch.zeros(pad)]).view(-1, LOSS_BLOCK)
    part = torch.zeros(LOSS_BLOCK)
    for row in grid:                      # thread t: t, t+1024, ...
        part = part + row
    s = LOSS_BLOCK // 2
    while s > 0:                          # binary tree
        part = part[:s] + part[s:2 * s]
        s //= 2
    return float(part[0] / torch.tensor(float(b)))
