"""fp32 model of the tile GRU kernels (k_gru_tile_fwd / k_gru_tile_bwd in
ops/hip/gru_kernels.hip) and the dalpha bound of their GPU test (CPU only).

The tile kernels run the recurrence of seq_reference.gru_fwd_ref /
gru_bwd_ref on the matrix cores. What sets them apart numerically from
the fp32 references is how the fp32 operand of each product (h, h_prev,
dpre_h) reaches the bf16 MFMA: as a sum of bf16 terms,

    hi = bf16(v),  lo = bf16(v - hi),  [lo2 = bf16(v - hi - lo)],

each multiplied by the bf16 weights in its own MFMA into an fp32
accumulator (forward: all terms into one, hi first; backward: hi into the
one seeded with the bias or `direct`, the remainder terms into a second
one that is added at the end). The model here does exactly that in fp32 torch arithmetic:
split operands, fp32 accumulation seeded with the bias (or `direct`), bf16
stores. tests/test_gru_tile_reference.py proves that the model alone meets
every limit tests/test_gpu_gru_tile.py holds the kernels to.

The split residual. bf16 keeps 8 significant bits, so for 2**e <= |v| <
2**(e+1) round-to-nearest gives |v - hi| <= 2**(e-8). d = v - hi is exact
in fp32: it is a multiple of v's last place 2**(e-23) and at most 2**(e-8),
16 bits. If |d| = 2**(e-8) it is a power of two and lo = d; otherwise d
lies in a binade e' <= e-9 and the second rounding leaves at most
2**(e'-8) <= 2**(e-17), so strictly

    |v - hi - lo| <= 2**(e-17) <= 2**-17 |v|                  (SPLIT_WORST)

attained only by a tie of the second rounding at the bottom of v's binade
(v = 1 + 2**-9 + 2**-17). SPLIT_REL = 2**-18 is the strict bound for the
upper half of every binade and twice the mean residual
(test_split_residual). What is left after two terms is again exact, a
multiple of 2**(e-23) below 2**(e-16): 8 bits, a bf16 value. Three terms
carry v exactly.

Forward: two terms (FWD_TERMS). The model stays within 7 e32 of the fp64
reference where a single rounding of h is off by thousands
(test_single_rounding_would_not_do).

Backward: three terms (BWD_TERMS). dh_t = carry + dh_out cancels, pn =
h_prev U_n^T + bh_n cancels, and every dpre is a product with one of them:
with two terms the 2**-17 residual of the carry and of pn, relative to
their absolute sums, becomes up to 28 bf16 ulps of dpre at these shapes
(test_two_terms_miss_the_backward_ulp_rule), with three the model is at
most one ulp off on under 0.02 % of the elements, as the fp32 reference.

The dalpha bound is gru_bwd_ref(with_bounds=True)'s recursion with two
terms added, as set for this kernel from the two-term residual,

    pn:     2**-18 (|h_prev| |U_n|^T)
    carry:  2**-18 (|dpre_h| |U|)

(slack for the three-term backward, whose operands are exact), and with
its two order-free summation terms counted for what the kernel adds, one
product per term and K index: (3H + 1) U32 instead of (H + 1) U32 behind
pn, (9H + 2) U32 instead of (3H + 2) U32 behind the carry. The
(terms) U32 sum|terms| form holds for any order of fp32 additions;
tests/dense_reference.py establishes exactness of the MFMA's fp32
accumulation only for integer data, so no tighter form is assumed.
"""
import torch

from tests import seq_reference as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U32 = R.U32
SPLIT_REL = 2.0 ** -18
SPLIT_WORST = 2.0 ** -17
FWD_TERMS = 2
BWD_TERMS = 3
MAX_H = 64

# (B, T, H): each as plain GRU and as AUGRU
TILE_SHAPES = [
    (1, 1, 33),     # one sample, one step, first width past the wave kernel
    (5, 2, 1),      # H = 1: one live column in one N tile
    (16, 3, 16),    # exactly one full tile, one N tile, K padded 16 -> 32
    (7, 5, 32),     # the wave kernel's top width through the tile path
    (17, 7, 36),    # one row into a second tile; reference DIEN; 16+16+4
    (15, 5, 48),    # one row short of a tile; K = 48 padded to 64
    (65, 4, 63),    # one sample into a second block; last column idle
    (9, 20, 64),    # the maximum width, longest chain
]
TILE_ALL = [(s, a) for s in TILE_SHAPES for a in (False, True)]
E2E_SHAPES = [s for s in TILE_SHAPES if s[2] in (36, 48, 63, 64)]


def split(v, terms=FWD_TERMS):
    """fp32 v -> its first `terms` bf16 terms, as fp32 tensors."""
    assert v.dtype == F32
    out, rest = [], v
    for _ in range(terms):
        out.append(rest.to(BF16).float())
        rest = rest - out[-1]
    return out


def split_matmul(v, w_t, seed, terms):
    """seed + hi @ w_t + lo @ w_t (+ ...) in fp32, the largest term first:
    one MFMA per term."""
    acc = seed
    for part in split(v, terms):
        acc = acc + part @ w_t
    return acc


def split_matmul_apart(v, w_t, big, small, terms):
    """The backward's form: big + hi @ w_t and small + (lo + ...) @ w_t
    kept apart, so that only the leading term's products round at the
    magnitude of the result; the caller adds the two once at the end."""
    parts = split(v, terms)
    big = big + parts[0] @ w_t
    for part in parts[1:]:
        small = small + part @ w_t
    return big, small


def tile_fwd_model(X3, U, bh, alpha):
    """gru_tile_fwd in fp32: returns h_out fp32 [B,T,H], gates bf16."""
    b, t, h3 = X3.shape
    hd = h3 // 3
    x3, u_t, bias = X3.float(), U.float().t().contiguous(), bh.float()
    h = torch.zeros(b, hd, dtype=F32)
    hs, gs = [], []
    for i in range(t):
        hp = split_matmul(h, u_t, bias, FWD_TERMS)
        xr, xz, xn = x3[:, i].split(hd, 1)
        hr, hz, hn = hp.split(hd, 1)
        r = torch.sigmoid(xr + hr)
        z = torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        hc = (1 - z) * n + z * h
        if alpha is not None:
            a = alpha[:, i:i + 1].float()
            h = (1 - a) * h + a * hc
        else:
            h = hc
        hs.append(h)
        gs.append(torch.cat([r, z, n], 1))
    return torch.stack(hs, 1), torch.stack(gs, 1).to(BF16)


def tile_bwd_model(dh_out, h_out, gates, U, bh, alpha, terms=BWD_TERMS):
    """gru_tile_bwd in fp32: (dpre_x bf16, dpre_h bf16, dalpha fp32|None).
    The carry is fed by the unrounded fp32 dpre_h parts, split."""
    b, t, hd = h_out.shape
    g3, u, bias = gates.float(), U.float(), bh.float()
    un_t = u[2 * hd:].t().contiguous()
    ho, dho = h_out.float(), dh_out.float()
    carry = torch.zeros(b, hd, dtype=F32)
    dpx = torch.zeros(b, t, 3 * hd, dtype=F32)
    dph = torch.zeros(b, t, 3 * hd, dtype=F32)
    da = torch.zeros(b, t, dtype=F32) if alpha is not None else None
    for i in range(t - 1, -1, -1):
        hp = ho[:, i - 1] if i > 0 else torch.zeros(b, hd, dtype=F32)
        r, z, n = g3[:, i].split(hd, 1)
        g = carry + dho[:, i]
        if alpha is not None:
            e = alpha[:, i:i + 1].float()
            hc = (1 - z) * n + z * hp
            da[:, i] = (g * (hc - hp)).sum(1)
        else:
            e = torch.ones(b, 1, dtype=F32)
        dn = g * e * (1 - z)
        dz = g * e * (hp - n)
        direct = g * ((1 - e) + e * z)
        dpn = dn * (1 - n * n)
        dpz = dz * z * (1 - z)
        pn, pn_small = split_matmul_apart(hp, un_t, bias[2 * hd:],
                                          torch.zeros(b, hd), terms)
        pn = pn + pn_small
        dpr = dpn * pn * r * (1 - r)
        dpn_h = dpn * r
        dpx[:, i] = torch.cat([dpr, dpz, dpn], 1)
        dph[:, i] = torch.cat([dpr, dpz, dpn_h], 1)
        carry, small = direct, torch.zeros(b, hd)
        for k in range(3):      # one gate (K block) at a time, as the kernel
            carry, small = split_matmul_apart(
                dph[:, i, k * hd:(k + 1) * hd], u[k * hd:(k + 1) * hd],
                carry, small, terms)
        carry = carry + small
    return dpx.to(BF16), dph.to(BF16), da


def tile_bwd_ref(dh_out, h_out, gates, U, bh, alpha):
    """fp64 gru_bwd_ref of the same inputs plus the per-element bound of
    dalpha for the tile kernel: seq_reference.gru_bwd_ref's recursion with
    the split residuals and the doubled summation terms of the module
    docstring. Returns (dpre_x, dpre_h, dalpha, dalpha_bound), unrounded."""
    dtype = F64
    b, t, hd = h_out.shape
    g3 = gates.to(dtype)
    u, bias = U.to(dtype), bh.to(dtype)
    ho, dho = h_out.to(dtype), dh_out.to(dtype)
    carry = torch.zeros(b, hd, dtype=dtype)
    c_err = torch.zeros(b, hd, dtype=dtype)
    dpx = torch.zeros(b, t, 3 * hd, dtype=dtype)
    dph = torch.zeros(b, t, 3 * hd, dtype=dtype)
    da = torch.zeros(b, t, dtype=dtype) if alpha is not None else None
    da_b = torch.zeros(b, t, dtype=dtype) if alpha is not None else None
    un = u[2 * hd:]
    for i in range(t - 1, -1, -1):
        hp = ho[:, i - 1] if i > 0 else torch.zeros(b, hd, dtype=dtype)
        r, z, n = g3[:, i].split(hd, 1)
        g = carry + dho[:, i]
        if alpha is not None:
            e = alpha[:, i:i + 1].to(dtype)
            hc = (1 - z) * n + z * hp
            da[:, i] = (g * (hc - hp)).sum(1)
        else:
            e = torch.ones(b, 1, dtype=dtype)
        cn = e * (1 - z)
        cz = e * (hp - n)
        cd = (1 - e) + e * z
        dpn = g * cn * (1 - n * n)
        dpz = g * cz * z * (1 - z)
        pn = hp @ un.t() + bias[2 * hd:]
        dpr = dpn * pn * r * (1 - r)
        dpn_h = dpn * r
        dpx[:, i] = torch.cat([dpr, dpz, dpn], 1)
        dph[:, i] = torch.cat([dpr, dpz, dpn_h], 1)
        carry_new = g * cd + dph[:, i] @ u
        # ---- the bound, term for term as in seq_reference.gru_bwd_ref
        ce = c_err + U32 * g.abs()
        if alpha is not None:
            diff = hc - hp
            ddiff = 4 * U32 * (((1 - z) * n).abs() + (z * hp).abs()
                               + hp.abs())
            da_b[:, i] = (ce * diff.abs() + g.abs() * ddiff).sum(1) \
                + (hd + 2) * U32 * (g * diff).abs().sum(1)
        kn = (cn * (1 - n * n)).abs()
        e_pn = ce * kn + 6 * U32 * dpn.abs()
        e_pz = ce * (cz * z * (1 - z)).abs() + 7 * U32 * dpz.abs()
        pn_abs = hp.abs() @ un.abs().t()
        dpn_pre = (BWD_TERMS * hd + 1) * U32 * (pn_abs + bias[2 * hd:].abs()) \
            + SPLIT_REL * pn_abs
        kr = (r * (1 - r)).abs()
        e_pr = (e_pn * pn.abs() + dpn.abs() * dpn_pre) * kr \
            + 4 * U32 * dpr.abs()
        e_pnh = e_pn * r.abs() + U32 * dpn_h.abs()
        e_h = torch.cat([e_pr, e_pz, e_pnh], 1)
        mv_abs = dph[:, i].abs() @ u.abs()
        c_err = ce * cd.abs() + 4 * U32 * (g * cd).abs() \
            + e_h @ u.abs() + (3 * BWD_TERMS * hd + 2) * U32 * ((g * cd).abs() + mv_abs) \
            + SPLIT_REL * mv_abs
        carry = carry_new
    return dpx, dph, da, da_b
