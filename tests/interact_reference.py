"""Reference and error bounds for the DLRM pair-dot interaction
(ops/hip/interact_kernels.hip and the scalar kernels in dense_kernels.hip).
No GPU needed.

The op, per sample, with X the [F, D] feature matrix:
    out[p(i, j)] = <X[i], X[j]>,  i < j,
    p(i, j) = i F - i (i + 1) / 2 + (j - i - 1)      (row-major upper triangle)
and its adjoint for an incoming g[P]:
    dX[i] = sum_{j != i} g[p(min(i, j), max(i, j))] X[j].
With the `cat` form, X = [bot; emb], the output row is [bot | out | zeros],
and dX[0] additionally gets the incoming gradient of the bot columns.

`ref_fwd` / `ref_bwd` work in whatever dtype they are given: int64 for the
exact cases, float64 for the rounding cases.

Bounds (u = 2^-24 for fp32, 2^-8 for the one rounding to bf16)
--------------------------------------------------------------
The kernels multiply bf16 values, whose products are exact in fp32, add
them in fp32 in some order, and round the sum once to bf16. A sum of n
terms t_k added in any order with n - 1 roundings is within
(n - 1) u sum|t_k| <= n u sum|t_k| of the exact sum (first order); the
final rounding adds 2^-8 |computed| <= 2^-8 (|ref| + that error).

    forward:   |out - ref| <= 2^-8 |ref| + D u sum_d |x_id x_jd| (1 + 2^-8)
    backward:  |dx  - ref| <= 2^-8 |ref| + F u (sum_j |s_ij x_jd| + |direct|)
                                              (1 + 2^-8)
(backward: F - 1 products plus the direct add of the cat form).

On integer inputs in [-2, 2] with D = 16, F <= 32 every forward dot is an
integer of magnitude <= 64 and every backward sum one of magnitude
<= 2 * 2 * 31 + 2 = 126: exact in fp32 in any order and exactly
representable in bf16, so the kernels must reproduce the integer reference
bit for bit.
"""
import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -8


def n_pairs(f):
    return f * (f - 1) // 2


def pair_rows_cols(f):
    iu = torch.triu_indices(f, f, offset=1)
    return iu[0], iu[1]


def ref_fwd(x):
    """x [B, F, D] -> [B, P] pair dots in x's dtype."""
    i, j = pair_rows_cols(x.shape[1])
    z = torch.bmm(x, x.transpose(1, 2))
    return z[:, i, j]


def pair_matrix(g, f):
    """g [B, >= P] -> symmetric S [B, F, F], zero diagonal. Columns of g
    past P are not read."""
    i, j = pair_rows_cols(f)
    s = torch.zeros(g.shape[0], f, f, dtype=g.dtype)
    s[:, i, j] = g[:, :n_pairs(f)]
    return s + s.transpose(1, 2)


def ref_bwd(g, x):
    """Hand-written adjoint of ref_fwd: g [B, >= P], x [B, F, D] -> dX."""
    return torch.bmm(pair_matrix(g, x.shape[1]), x)


def ref_cat_fwd(bot, emb, p_pad):
    """[bot | pair dots over [bot; emb] | zeros] -> [B, D + p_pad]."""
    x = torch.cat([bot.unsqueeze(1), emb], dim=1)
    out = ref_fwd(x)
    pad = torch.zeros(out.shape[0], p_pad - out.shape[1], dtype=out.dtype)
    return torch.cat([bot, out, pad], dim=1)


def ref_cat_bwd(grad, bot, emb):
    """grad [B, D + p_pad] -> (dbot, demb)."""
    d = bot.shape[1]
    x = torch.cat([bot.unsqueeze(1), emb], dim=1)
    dx = ref_bwd(grad[:, d:], x)
    return dx[:, 0] + grad[:, :d], dx[:, 1:]


def fwd_bound(x):
    """Bound on |out - ref_fwd(x)|, [B, P]; x fp64 holding bf16 values."""
    x = x.double()
    a = x.abs()
    i, j = pair_rows_cols(x.shape[1])
    ref = ref_fwd(x)
    mag = torch.bmm(a, a.transpose(1, 2))[:, i, j]
    return UBF * ref.abs() + x.shape[2] * U32 * mag * (1 + UBF)


def bwd_bound(g, x, direct=None):
    """Bound on |dx - ref|, [B, F, D]; `direct` [B, D] is the cat form's
    incoming gradient of the bot columns (added to row 0)."""
    g, x = g.double(), x.double()
    f = x.shape[1]
    ref = ref_bwd(g, x)
    mag = torch.bmm(pair_matrix(g, f).abs(), x.abs())
    if direct is not None:
        ref = ref.clone()
        ref[:, 0] += direct.double()
        mag[:, 0] += direct.double().abs()
    return UBF * ref.abs() + f * U32 * mag * (1 + UBF)


def int_tensor(shape, seed):
    """Integers in [-2, 2], int64."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=gen, dtype=torch.int64)


def nonzero_int_tensor(shape, seed):
    """Integers in {-2, -1, 1, 2}, int64 (for the grad's pad columns)."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randint(1, 3, shape, generator=gen, dtype=torch.int64)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64)
    return v * (2 * sign - 1)
