"""fp64 references and derived error bounds for the sequence kernels
(CPU only): attention (k_mha_*), GRU / AUGRU (k_gru_*), residual LayerNorm
(k_resln_*), L2 normalize (k_l2norm_*), DIN features (k_din_feat_*) and the
masked softmax pool (k_msm_pool_*).

Every reference takes exactly what the kernel is handed — bf16-representable
q, k, v, dout, X3, U, gates, z, and fp32 for the rest — so the only error
left in a comparison is the kernel's own. The backward references are the
explicit formulas, not autograd of the forward; tests/test_seq_reference.py
proves them against fp64 autograd and torch's own ops without a GPU, and
tests/test_gpu_seq_kernels.py runs the kernels on the cases below.

All bounds follow tests/dense_reference.py's linear_bounds:
  * one output rounding, BF * |ref| for a bf16 output, none for fp32;
  * fp32 arithmetic: a sum of `red` terms is off by at most
    red * U32 * sum|terms| whatever its order (tree, atomics, FMA), one
    product or sum by U32 * |result|;
  * EXP_REL per probability where the kernel uses __expf, for |x| <= EXP_ARG
    (asserted by exp_precondition on the reference's own argument);
  * RSQRT_REL for the hardware reciprocal square root.
Each reference is generic over `dtype`: evaluated in fp32 on the CPU it has
to stay inside its own bound (test_seq_reference.py), which is what shows a
bound is not too tight for an honest fp32 implementation.
"""
import functools
import math

import torch

from tests.dense_reference import GUARD, carve  # noqa: F401  (re-exported)

BF16 = torch.bfloat16
F64 = torch.float64
F32 = torch.float32

U32 = 2.0 ** -23        # fp32 spacing of 1.0: bound of one fp32 rounding
BF = 2.0 ** -8          # bf16 spacing of 1.0: bound of one bf16 rounding
# __expf(x) is a hardware exp2 of x * log2(e): the product carries a
# relative error of 2**-24, which exp2 turns into |x| * 2**-24 relative,
# plus 1 ulp of the exp2 unit. For |x| <= 32 that is below 2**-18.
EXP_REL = 2.0 ** -18
EXP_ARG = 32.0
# v_rsq_f32 is accurate to 1 ulp; rsqrtf may refine or not: allow 2 ulp
RSQRT_REL = 2.0 ** -22
FLIP_CAP = 0.01         # share of bf16 outputs that may be 1 ulp off
# the row max k_mha_fwd stores for a row with no live key: fp32(-1e30)
MHA_DEAD_MAX = float(torch.tensor(-1e30, dtype=torch.float32))

# ------------------------------------------------------------------ cases

# (B, T, D, H)
MHA_SHAPES = [
    (3, 1, 4, 1),       # T = 1, one head of dh = 4
    (2, 17, 16, 4),     # dh = 4
    (2, 20, 64, 8),     # dh = 8
    (2, 7, 16, 1),      # dh = 16
    (2, 33, 64, 2),     # dh = 32; T*H = 66 crosses one wave
    (1, 128, 32, 8),    # T*H = 1024: the largest block, B = 1
    (5, 51, 32, 4),     # the BST shape
]
# none: no pads; random: 40 % pads, >= 1 live key per sample; last: only
# the last key live; dead: sample 0 fully padded, the others as `random`
MHA_PADS = ["none", "random", "last", "dead"]

# (B, T, H); each as plain GRU and as AUGRU
GRU_SHAPES = [
    (1, 1, 32),     # one sample, one step: three idle waves in the block
    (5, 2, 1),      # H = 1; B = 5: a second block with one live wave
    (6, 7, 8),
    (7, 5, 21),     # 3H = 63: the last lane of rep 0 idle
    (7, 5, 22),     # 3H = 66: two gates in rep 1
    (9, 20, 32),    # the DIEN width, 3H = 96
]
GRU_IN = 20         # input width of the end-to-end FusedGRU cases

RESLN_BWD_STRIDE_M = 64 * 256 + 5       # backward grid-stride loop
RESLN_FWD_STRIDE_M = 4096 * 256 + 3     # forward grid-stride loop
# (M, N)
RESLN_SHAPES = [(m, n) for n in (16, 32, 64) for m in (1, 257)] + [
    (RESLN_BWD_STRIDE_M, 32), (RESLN_FWD_STRIDE_M, 16)]

L2NORM_SHAPES = [(1, 1), (5, 65), (6, 100), (257, 16)]   # (M, N)
L2NORM_EPS = 1e-12

# (B, T, D); the last one is above the 8192-block * 256-thread grid cap
DIN_SHAPES = [(1, 1, 1), (33, 17, 32), (1025, 64, 32)]
DIN_RANGE = 15

# (B, T, D); the block is 128 threads: T > 128 and D > 128 loop
MSM_SHAPES = [(1, 1, 1), (3, 129, 32), (3, 50, 130), (2, 300, 8)]


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def randn_bf16(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF16)


def bf16_ulp(x):
    """Spacing of the bf16 grid at |x| (x already on the grid), fp64."""
    x = x.double().abs()
    e = torch.floor(torch.log2(torch.clamp(x, min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 7)


def ulp_flips(got_bf16, ref64):
    """(max distance in bf16 ulps, share of elements that differ) between a
    bf16 tensor and the fp64 reference rounded to bf16."""
    want = ref64.float().to(BF16)
    g, w = got_bf16.double(), want.double()
    diff = (g - w).abs()
    ulp = torch.maximum(bf16_ulp(g), bf16_ulp(w))
    n_ulp = float((diff / ulp).max()) if diff.numel() else 0.0
    share = float((diff != 0).double().mean()) if diff.numel() else 0.0
    return n_ulp, share


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    den = float(ref.norm())
    if den == 0.0:
        return 0.0 if float(got.norm()) == 0.0 else float("inf")
    return float((got - ref).norm()) / den


def exp_precondition(arg, live=None):
    """The fast-exponential allowance holds for |x| <= EXP_ARG."""
    a = arg.abs() if live is None else torch.where(
        live, arg.abs(), torch.zeros_like(arg))
    return float(a.max()) <= EXP_ARG if a.numel() else True


# -------------------------------------------------------------- attention

@functools.lru_cache(maxsize=None)
def mha_pad(b, t, pattern):
    gen = _gen(b, t, len(pattern), 5)
    rnd = torch.rand(b, t, generator=gen) < 0.4
    keep = torch.randint(0, t, (b,), generator=gen)
    rnd[torch.arange(b), keep] = False
    if pattern == "none":
        return torch.zeros(b, t, dtype=torch.bool)
    if pattern == "random":
        return rnd
    if pattern == "last":
        pad = torch.ones(b, t, dtype=torch.bool)
        pad[:, -1] = False
        return pad
    assert pattern == "dead"
    rnd[0] = True
    return rnd


@functools.lru_cache(maxsize=None)
def mha_case(b, t, d, h):
    gen = _gen(b, t, d, h)
    return {"q": randn_bf16(gen, b, t, d), "k": randn_bf16(gen, b, t, d),
            "v": randn_bf16(gen, b, t, d), "dout": randn_bf16(gen, b, t, d),
            "scale": 1.0 / math.sqrt(d // h)}


def _heads(x, h, dtype):
    b, t, d = x.shape
    return x.to(dtype).view(b, t, h, d // h).transpose(1, 2)   # [B,H,T,dh]


def _unheads(x):
    b, h, t, dh = x.shape
    return x.transpose(1, 2).reshape(b, t, h * dh)


def mha_ref(q, k, v, pad, h, scale, dout=None, dtype=F64):
    """Masked softmax attention and, with dout, its backward:
        p = softmax_t(q.k_t * scale | live t),  out = sum_t p_t v_t
        dp_t = dout.v_t,  rd = sum_t p_t dp_t,  ds_t = p_t (dp_t - rd) scale
        dq = sum_t ds_t k_t;  dk_t = sum_q ds_qt q_q;  dv_t = sum_q p_qt dout_q
    A sample with no live key gives zeros everywhere (stats: max -1e30,
    sum 0). Returns a dict that also holds the intermediates the bound
    functions need."""
    qs, ks, vs = (_heads(x, h, dtype) for x in (q, k, v))
    live = (~pad)[:, None, None, :].expand(-1, h, q.shape[1], -1)
    s = qs @ ks.transpose(-1, -2) * scale
    neg = torch.full_like(s, MHA_DEAD_MAX)
    mx = torch.where(live, s, neg).amax(-1, keepdim=True)
    arg = torch.where(live, s - mx, torch.zeros_like(s))
    e = torch.where(live, torch.exp(arg), torch.zeros_like(s))
    ssum = e.sum(-1, keepdim=True)
    p = e / torch.clamp(ssum, min=1e-20)
    r = {"out": _unheads(p @ vs), "p": p, "e": e, "arg": arg, "live": live,
         "stats": torch.cat([mx, ssum], -1),       # [B,H,T,2]
         "qs": qs, "ks": ks, "vs": vs}
    if dout is not None:
        gs = _heads(dout, h, dtype)
        dp = gs @ vs.transpose(-1, -2)
        rd = (p * dp).sum(-1, keepdim=True)
        ds = p * (dp - rd) * scale
        r.update(gs=gs, dp=dp, rd=rd, ds=ds, dq=_unheads(ds @ ks),
                 dk=_unheads(ds.transpose(-1, -2) @ qs),
                 dv=_unheads(p.transpose(-1, -2) @ gs))
    return r


def mha_bounds(r, scale):
    """Per-element bounds from an fp64 mha_ref result.

    score: a dh-term fp32 dot times scale, minus the max:
        ds_t <= U32 ((dh + 1) scale |q|.|k_t| + |arg_t|)
    which exp turns into a relative error of e_t; with the fast exp,
        eps_t = EXP_REL + ds_t.
    The row max is off by dmx <= max_t ds_t; it cancels in p as long as
    sum is built on the same max. sum over T terms:
        dsum <= sum_t e_t (eps_t + dmx) + T U32 sum
    out = acc / sum: each p_t is off by p_t (eps_t + epsrow) with
        epsrow = sum_t p_t eps_t + (T + 2) U32   (relative error of sum),
        dout <= BF |out| + sum_t p_t (eps_t + epsrow) |v_t|
                + (T + 2) U32 sum_t p_t |v_t|
    backward, with eta_t = eps_t + epsrow + 2 U32 the relative error of
    the recomputed p_t = exp(.) * (1 / sum):
        ddp_t <= dh U32 |dout|.|v_t|
        drd   <= sum_t p_t (eta_t |dp_t| + ddp_t) + T U32 sum_t p_t |dp_t|
        dds_t <= scale p_t (eta_t |dp_t - rd| + ddp_t + drd
                            + 3 U32 |dp_t - rd|)
        ddq   <= BF |dq| + sum_t (dds_t + T U32 |ds_t|) |k_t|
        ddk_t <= BF |dk_t| + sum_q (dds_qt + T U32 |ds_qt|) |q_q|
        ddv_t <= BF |dv_t| + sum_q p_qt (eta_qt + T U32) |dout_q|
    """
    qs, ks, vs, p, e = r["qs"], r["ks"], r["vs"], r["p"], r["e"]
    t, dh = qs.shape[2], qs.shape[3]
    sabs = qs.abs() @ ks.abs().transpose(-1, -2) * scale
    dsc = torch.where(r["live"], U32 * ((dh + 1) * sabs + r["arg"].abs()),
                      torch.zeros_like(sabs))
    eps = EXP_REL + dsc
    dmx = dsc.amax(-1, keepdim=True)
    ssum = r["stats"][..., 1:2]
    b = {"mx": dmx.squeeze(-1),
         "sum": ((e * (eps + dmx)).sum(-1, keepdim=True)
                 + t * U32 * ssum).squeeze(-1)}
    epsrow = (p * eps).sum(-1, keepdim=True) + (t + 2) * U32
    vabs = vs.abs()
    b["out"] = BF * r["out"].abs() + _unheads(
        (p * (eps + epsrow)) @ vabs + (t + 2) * U32 * (p @ vabs))
    if "ds" in r:
        gs, dp, rd, ds = r["gs"], r["dp"], r["rd"], r["ds"]
        eta = eps + epsrow + 2 * U32
        ddp = dh * U32 * (gs.abs() @ vabs.transpose(-1, -2))
        drd = (p * (eta * dp.abs() + ddp)).sum(-1, keepdim=True) \
            + t * U32 * (p * dp.abs()).sum(-1, keepdim=True)
        dds = scale * p * (eta * (dp - rd).abs() + ddp + drd
                           + 3 * U32 * (dp - rd).abs())
        w = dds + t * U32 * ds.abs()
        b["dq"] = BF * r["dq"].abs() + _unheads(w @ ks.abs())
        b["dk"] = BF * r["dk"].abs() + _unheads(
            w.transpose(-1, -2) @ qs.abs())
        b["dv"] = BF * r["dv"].abs() + _unheads(
            (p * (eta + t * U32)).transpose(-1, -2) @ gs.abs())
    return b


# -------------------------------------------------------------------- GRU

@functools.lru_cache(maxsize=None)
def gru_case(b, t, h, augru):
    """What gru_fwd is handed (X3, U bf16; bh, alpha fp32) plus the inputs
    of the end-to-end cases (x, W_ih bf16-representable, b_ih fp32) that X3
    is made of, and the upstream gradient of h_out."""
    gen = _gen(b, t, h, int(augru))
    std = 1.0 / math.sqrt(h)
    uni = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1) * std  # noqa
    c = {"x": randn_bf16(gen, b, t, GRU_IN),
         "w_ih": uni(3 * h, GRU_IN).to(BF16), "b_ih": uni(3 * h),
         "U": uni(3 * h, h).to(BF16), "bh": uni(3 * h),
         "dh_out": torch.randn(b, t, h, generator=gen),
         "alpha": torch.rand(b, t, generator=gen) if augru else None}
    x3 = c["x"].double() @ c["w_ih"].double().t() + c["b_ih"].double()
    c["X3"] = x3.float().to(BF16)
    return c


def gru_fwd_ref(X3, U, bh, alpha, dtype=F64):
    """torch GRU cell ([r; z; n] rows) with the optional attention gate:
        r = sig(x_r + U_r h + bh_r), z = sig(x_z + U_z h + bh_z)
        n = tanh(x_n + r (U_n h + bh_n)), hc = (1 - z) n + z h
        h' = hc                      (GRU)
        h' = (1 - a) h + a hc        (AUGRU)
    Returns h_out [B,T,H] and the unrounded gates [B,T,3H]."""
    b, t, h3 = X3.shape
    hd = h3 // 3
    x3, u, bias = X3.to(dtype), U.to(dtype), bh.to(dtype)
    h = torch.zeros(b, hd, dtype=dtype)
    hs, gs = [], []
    for i in range(t):
        hp = h @ u.t() + bias
        xr, xz, xn = x3[:, i].split(hd, 1)
        hr, hz, hn = hp.split(hd, 1)
        r = torch.sigmoid(xr + hr)
        z = torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        hc = (1 - z) * n + z * h
        if alpha is not None:
            a = alpha[:, i:i + 1].to(dtype)
            h = (1 - a) * h + a * hc
        else:
            h = hc
        hs.append(h)
        gs.append(torch.cat([r, z, n], 1))
    return torch.stack(hs, 1), torch.stack(gs, 1)


def gru_bwd_ref(dh_out, h_out, gates, U, bh, alpha, dtype=F64,
                with_bounds=False):
    """gru_bwd's inputs -> (dpre_x, dpre_h, dalpha), unrounded. Per step,
    going back, with g = dh_out_t + carry, e = alpha_t (1 for GRU):
        dalpha = sum_k g (hc - h_prev)
        dn = g e (1 - z), dz = g e (h_prev - n), direct = g ((1 - e) + e z)
        dpn = dn (1 - n^2), dpz = dz z (1 - z)
        pn = U_n h_prev + bh_n, dpr = dpn pn r (1 - r)
        dpre_x = [dpr, dpz, dpn];  dpre_h = [dpr, dpz, dpn r]
        carry = direct + dpre_h U
    with_bounds adds a running per-element fp32 error bound of dalpha
    (the only fp32 output): every quantity is linear in g, so an error c of
    g is passed on through the absolute values of the same coefficients,
    each product chain adds K U32 |result| (K = its number of roundings),
    the H-term dot of pn adds (H + 1) U32 (|U_n| |h_prev| + |bh_n|), and
    the 3H-term transposed matvec adds (3H + 2) U32 of its absolute sum."""
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
        if with_bounds:
            ce = c_err + U32 * g.abs()            # the add of dh_out
            if alpha is not None:
                diff = hc - hp
                ddiff = 4 * U32 * (((1 - z) * n).abs() + (z * hp).abs()
                                   + hp.abs())
                da_b[:, i] = (ce * diff.abs() + g.abs() * ddiff).sum(1) \
                    + (hd + 2) * U32 * (g * diff).abs().sum(1)
            kn = (cn * (1 - n * n)).abs()
            e_pn = ce * kn + 6 * U32 * dpn.abs()
            e_pz = ce * (cz * z * (1 - z)).abs() + 7 * U32 * dpz.abs()
            dpn_pre = (hd + 1) * U32 * (hp.abs() @ un.abs().t()
                                        + bias[2 * hd:].abs())
            kr = (r * (1 - r)).abs()
            e_pr = (e_pn * pn.abs() + dpn.abs() * dpn_pre) * kr \
                + 4 * U32 * dpr.abs()
            e_pnh = e_pn * r.abs() + U32 * dpn_h.abs()
            e_h = torch.cat([e_pr, e_pz, e_pnh], 1)
            c_err = ce * cd.abs() + 4 * U32 * (g * cd).abs() \
                + e_h @ u.abs() + (3 * hd + 2) * U32 * (
                    (g * cd).abs() + dph[:, i].abs() @ u.abs())
        carry = carry_new
    if with_bounds:
        return dpx, dph, da, da_b
    return dpx, dph, da


def gru_chain(c, rounded, dtype=F64):
    """End-to-end gradients of sum(h_out * dh_out) w.r.t. x, W_ih, b_ih,
    W_hh, b_hh (and alpha), by the explicit formulas and the GEMMs of
    FusedGRU's backward. rounded = False keeps everything in fp64 (must
    equal autograd); rounded = True rounds to bf16 what the kernels store
    in bf16 — the gates, dpre_x, dpre_h and the h_prev operand of the
    W_hh GEMM — and is the model of the storage noise."""
    rnd = (lambda v: v.float().to(BF16).to(dtype)) if rounded \
        else (lambda v: v)
    h_out, gates = gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"], dtype)
    dpx, dph, da = gru_bwd_ref(c["dh_out"], h_out, rnd(gates), c["U"],
                               c["bh"], c["alpha"], dtype)
    b, t, hd = h_out.shape
    dpx2 = rnd(dpx).reshape(b * t, 3 * hd)
    dph2 = rnd(dph).reshape(b * t, 3 * hd)
    x2 = c["x"].to(dtype).reshape(b * t, -1)
    hprev = rnd(torch.cat([torch.zeros(b, 1, hd, dtype=dtype),
                           h_out[:, :-1]], 1)).reshape(b * t, hd)
    out = {"x": (dpx2 @ c["w_ih"].to(dtype)).reshape(b, t, -1),
           "w_ih": dpx2.t() @ x2, "b_ih": dpx2.sum(0),
           "w_hh": dph2.t() @ hprev, "b_hh": dph2.sum(0)}
    if da is not None:
        out["alpha"] = da
    return out


def gru_autograd(c):
    """fp64 autograd of the forward with the bf16 roundings of x, W and X3
    applied (X3's rounding passes the gradient straight through)."""
    leaf = lambda v: v.double().clone().requires_grad_(True)  # noqa: E731
    p = {"x": leaf(c["x"]), "w_ih": leaf(c["w_ih"]), "b_ih": leaf(c["b_ih"]),
         "w_hh": leaf(c["U"]), "b_hh": leaf(c["bh"])}
    if c["alpha"] is not None:
        p["alpha"] = leaf(c["alpha"])
    b, t, _ = c["x"].shape
    x3 = p["x"] @ p["w_ih"].t() + p["b_ih"]
    x3 = x3 + (c["X3"].double() - x3).detach()
    hd = c["U"].shape[1]
    h = torch.zeros(b, hd, dtype=F64)
    hs = []
    for i in range(t):
        hp = h @ p["w_hh"].t() + p["b_hh"]
        xr, xz, xn = x3[:, i].split(hd, 1)
        hr, hz, hn = hp.split(hd, 1)
        r = torch.sigmoid(xr + hr)
        z = torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        hc = (1 - z) * n + z * h
        if "alpha" in p:
            a = p["alpha"][:, i:i + 1]
            h = (1 - a) * h + a * hc
        else:
            h = hc
        hs.append(h)
    h_out = torch.stack(hs, 1)
    (h_out * c["dh_out"].double()).sum().backward()
    return h_out.detach(), {k: v.grad for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def gru_storage_noise(b, t, h, augru):
    """Relative L2 deviation, per gradient tensor, of the bf16-storing
    chain from fp64 autograd: what rounding the gates, dpre and h_prev to
    bf16 costs, with every other operation exact."""
    c = gru_case(b, t, h, augru)
    _, ref = gru_autograd(c)
    got = gru_chain(c, rounded=True)
    return {k: rel_l2(got[k], ref[k]) for k in got}


# ------------------------------------------------------ residual LayerNorm

RESLN_EPS = 1e-5


@functools.lru_cache(maxsize=4)
def resln_case(m, n):
    gen = _gen(m, n, 3)
    return {"x": randn_bf16(gen, m, n, scale=2.0),
            "a": randn_bf16(gen, m, n),
            "gamma": 1.5 * torch.ones(n) + 0.1 * torch.randn(n, generator=gen),
            "beta": 0.05 + 0.1 * torch.randn(n, generator=gen),
            "dy": randn_bf16(gen, m, n)}


def resln_fwd_ref(x, a, gamma, beta, eps=RESLN_EPS, dtype=F64):
    z = x.to(dtype) + a.to(dtype)
    mean = z.mean(1, keepdim=True)
    d = z - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * gamma.to(dtype) + beta.to(dtype)
    return {"y": y, "z": z, "stats": torch.cat([mean, rstd], 1),
            "d": d, "var": var}


def resln_fwd_bounds(r, gamma, beta, eps=RESLN_EPS):
    """z: one fp32 add, then the bf16 store: (BF + U32) |z|.
    mean: an N-term sum: dmean <= (N + 1) U32 mean|z|.
    d = z - mean: dd <= dmean + U32 (|z| + |d|).
    var = mean(d^2): dvar <= mean(2 |d| dd) + (N + 2) U32 var.
    rstd = rsqrt(var + eps): relative 0.5 dvar / (var + eps) + RSQRT_REL
    + U32.  y = d rstd gamma + beta:
        dy <= BF |y| + |gamma| rstd dd + |d rstd gamma| rel(rstd)
              + 3 U32 (|d rstd gamma| + |beta|)"""
    z, d, var = r["z"], r["d"], r["var"]
    n = z.shape[1]
    mean, rstd = r["stats"][:, :1], r["stats"][:, 1:]
    dmean = (n + 1) * U32 * z.abs().mean(1, keepdim=True)
    dd = dmean + U32 * (z.abs() + d.abs())
    dvar = (2 * d.abs() * dd).mean(1, keepdim=True) + (n + 2) * U32 * var
    rel = 0.5 * dvar / (var + eps) + RSQRT_REL + U32
    core = (d * rstd * gamma.double()).abs()
    return {"z": (BF + U32) * z.abs(),
            "stats": torch.cat([dmean, rstd * rel], 1),
            "y": BF * r["y"].abs() + gamma.double().abs() * rstd * dd
            + core * rel + 3 * U32 * (core + beta.double().abs())}


def resln_bwd_depth(m):
    """Longest chain of fp32 additions behind one dgamma / dbeta element —
    the launch shape of resln_bwd in ops/hip/dense_kernels.hip: each thread
    sums its rows in a register, 256 threads merge in LDS, the blocks merge
    in global memory."""
    blocks = max(min((m + 2047) // 2048, 4096), 64)
    rows = (m + blocks * 256 - 1) // (blocks * 256)
    return rows + 256 + blocks


def resln_bwd_ref(dy, z16, stats, gamma, dtype=F64):
    """resln_bwd's inputs (bf16 dy and z, fp32 stats and gamma):
        xh = (z - mean) rstd, gg = dy gamma
        s1 = mean(gg), s2 = mean(gg xh)
        dz = (gg - s1 - xh s2) rstd
        dgamma = sum_rows dy xh, dbeta = sum_rows dy"""
    g, z = dy.to(dtype), z16.to(dtype)
    mean, rstd = stats[:, :1].to(dtype), stats[:, 1:].to(dtype)
    xh = (z - mean) * rstd
    gg = g * gamma.to(dtype)
    s1 = gg.mean(1, keepdim=True)
    s2 = (gg * xh).mean(1, keepdim=True)
    return {"dz": (gg - s1 - xh * s2) * rstd, "dgamma": (g * xh).sum(0),
            "dbeta": g.sum(0), "xh": xh, "gg": gg, "s1": s1, "s2": s2,
            "g": g, "rstd": rstd}


def resln_bwd_bounds(r):
    """xh: an exact-input subtraction and a product: 2 U32 |xh|.
    s1, s2: N-term sums of products: (N + 3) U32 mean|terms| (+ the error
    of xh inside s2). dz: three terms, each carrying its inputs' errors,
    two subtractions and the product with rstd, then the bf16 store.
    dgamma / dbeta: sums over M rows in a chain of resln_bwd_depth(M)
    additions: depth U32 sum|terms| (+ the error of xh)."""
    xh, gg, s1, s2, g, rstd = (r[k] for k in ("xh", "gg", "s1", "s2", "g",
                                              "rstd"))
    m, n = xh.shape
    dxh = 2 * U32 * xh.abs()
    ds1 = (n + 3) * U32 * gg.abs().mean(1, keepdim=True)
    ds2 = (n + 3) * U32 * (gg * xh).abs().mean(1, keepdim=True) \
        + (gg.abs() * dxh).mean(1, keepdim=True)
    mag = gg.abs() + s1.abs() + (xh * s2).abs()
    inner = U32 * gg.abs() + ds1 + xh.abs() * ds2 + s2.abs() * dxh \
        + 4 * U32 * mag
    depth = resln_bwd_depth(m)
    return {"dz": BF * r["dz"].abs() + inner * rstd,
            "dgamma": (depth + 2) * U32 * (g * xh).abs().sum(0)
            + (g.abs() * dxh).sum(0),
            "dbeta": depth * U32 * g.abs().sum(0)}


# ---------------------------------------------------------------- l2norm

@functools.lru_cache(maxsize=None)
def l2norm_case(m, n):
    gen = _gen(m, n, 7)
    x = randn_bf16(gen, m, n)
    if m >= 5:
        x[3] = 0            # one all-zero row
    return {"x": x, "dy": randn_bf16(gen, m, n)}


def l2norm_fwd_ref(x, eps=L2NORM_EPS, dtype=F64):
    xv = x.to(dtype)
    ss = (xv * xv).sum(1, keepdim=True)
    inv = 1.0 / torch.sqrt(torch.clamp(ss, min=eps))
    return {"y": xv * inv, "inv": inv.squeeze(1), "ss": ss}


def _wave_terms(n):
    """Additions behind a 64-lane strided sum of n terms."""
    return (n + 63) // 64 + 6 + 1


def l2norm_fwd_bounds(r):
    """ss: (lane terms + 6 shuffle steps + the squares) U32 ss, relative;
    inv = rsqrt: half of that plus RSQRT_REL; y = x inv: one more product
    and the bf16 store. A row clamped at eps has an exact argument."""
    n = r["y"].shape[1]
    rel = 0.5 * _wave_terms(n) * U32 + RSQRT_REL
    return {"inv": r["inv"] * rel,
            "y": (BF + rel + U32) * r["y"].abs()}


def l2norm_bwd_ref(dy, y16, inv, dtype=F64):
    """dx = (dy - y <y, dy>) inv from the bf16 y and fp32 inv the forward
    stored."""
    g, y = dy.to(dtype), y16.to(dtype)
    dot = (y * g).sum(1, keepdim=True)
    return {"dx": (g - y * dot) * inv.to(dtype)[:, None], "dot": dot,
            "g": g, "y": y, "inv": inv.to(dtype)[:, None]}


def l2norm_bwd_bounds(r):
    """dot: wave sum of products: terms U32 sum|y dy|. dx: the product
    y dot, the subtraction and the product with inv (3 roundings of the
    magnitudes involved), then the bf16 store."""
    n = r["y"].shape[1]
    ddot = _wave_terms(n) * U32 * (r["y"] * r["g"]).abs().sum(1, keepdim=True)
    mag = r["g"].abs() + (r["y"] * r["dot"]).abs()
    return {"dx": BF * r["dx"].abs()
            + r["inv"] * (r["y"].abs() * ddot + 3 * U32 * mag)}


# -------------------------------------------------------------- din_feat

@functools.lru_cache(maxsize=2)
def din_case(b, t, d):
    """Integer operands with |s|, |t|, |g| <= 15: every product is at most
    225 and every sum far below 2**24, so fwd and both backward kernels are
    exact and int64 arithmetic is the reference."""
    gen = _gen(b, t, d, 11)
    ri = lambda *s: torch.randint(-DIN_RANGE, DIN_RANGE + 1, s,  # noqa: E731
                                  generator=gen)
    seq, tgt, g = ri(b, t, d), ri(b, d), ri(b * t, 4 * d)
    te = tgt[:, None, :].expand(b, t, d)
    out = torch.cat([seq, te, seq - te, seq * te], 2).reshape(b * t, 4 * d)
    # the same in floating point: an IEEE product of a negative number and
    # zero is -0, which int64 cannot say and a bit-exact comparison sees
    sf, tf = seq.double(), te.double()
    out_f = torch.cat([sf, tf, sf - tf, sf * tf], 2).reshape(b * t, 4 * d)
    g4 = g.view(b, t, 4, d)
    dseq = g4[:, :, 0] + g4[:, :, 2] + g4[:, :, 3] * te
    dtgt = (g4[:, :, 1] - g4[:, :, 2] + g4[:, :, 3] * seq).sum(1)
    return {"seq": seq, "tgt": tgt, "g": g, "out": out, "out_f": out_f,
            "dseq": dseq, "dtgt": dtgt}


# -------------------------------------------------------------- msm_pool

@functools.lru_cache(maxsize=None)
def msm_case(b, t, d):
    gen = _gen(b, t, d, 13)
    mask = torch.rand(b, t, generator=gen) > 0.3
    mask[:, t // 2] = True
    return {"scores": torch.randn(b, t, generator=gen) * 2,
            "seq": torch.randn(b, t, d, generator=gen),
            "mask": mask, "dout": torch.randn(b, d, generator=gen)}


def msm_fwd_ref(scores, seq, mask, dtype=F64):
    """w = softmax of the scores over the valid positions (0 elsewhere and
    on a row with none), out = w @ seq."""
    s = scores.to(dtype)
    mx = torch.where(mask, s, torch.full_like(s, -3.4e38)).amax(
        1, keepdim=True)
    arg = torch.where(mask, s - mx, torch.zeros_like(s))
    e = torch.where(mask, torch.exp(arg), torch.zeros_like(s))
    ssum = e.sum(1, keepdim=True)
    w = e / (ssum + 1e-20)
    return {"w": w, "out": (w[:, :, None] * seq.to(dtype)).sum(1),
            "arg": arg}


def msm_fwd_bounds(r, seq, mask):
    """e_t: EXP_REL + U32 |arg_t| (the subtraction). sum: T terms, each
    off by its e_t's error: relative epsrow = sum_t w_t eps_t + (T + 1)
    U32. w_t = e_t (1 / sum): w_t (eps_t + epsrow + 2 U32).
    out_d = sum_t w_t seq_td: sum_t dw_t |seq_td| + T U32 sum_t w_t
    |seq_td|."""
    w = r["w"]
    t = w.shape[1]
    eps = EXP_REL + U32 * r["arg"].abs()
    epsrow = (w * eps).sum(1, keepdim=True) + (t + 1) * U32
    dw = w * (eps + epsrow + 2 * U32)
    sabs = seq.double().abs()
    return {"w": dw,
            "out": (dw[:, :, None] * sabs).sum(1)
            + t * U32 * (w[:, :, None] * sabs).sum(1)}


def msm_bwd_ref(dout, seq, w32, mask, dtype=F64):
    """msm_pool_bwd's inputs (all fp32):
        sdot_t = dout . seq_t, wdot = sum_t w_t sdot_t
        dscores_t = w_t (sdot_t - wdot) on valid t, 0 elsewhere
        dseq_t = w_t dout"""
    g, q, w = dout.to(dtype), seq.to(dtype), w32.to(dtype)
    sdot = (q * g[:, None, :]).sum(2)
    wdot = (w * sdot).sum(1, keepdim=True)
    ds = torch.where(mask, w * (sdot - wdot), torch.zeros_like(w))
    return {"dscores": ds, "dseq": w[:, :, None] * g[:, None, :],
            "sdot": sdot, "wdot": wdot, "w": w, "g": g, "q": q}


def msm_bwd_bounds(r, mask):
    """sdot: D-term dot: dsdot <= (D + 1) U32 |dout| . |seq_t|.
    wdot: dwdot <= sum_t w_t dsdot_t + (T + 1) U32 sum_t |w_t sdot_t|.
    dscores: w_t (dsdot_t + dwdot) + 2 U32 w_t (|sdot_t| + |wdot|).
    dseq: one product: U32 |dseq|."""
    w, sdot, wdot = r["w"], r["sdot"], r["wdot"]
    t, d = r["q"].shape[1], r["q"].shape[2]
    dsdot = (d + 1) * U32 * (r["q"].abs() * r["g"].abs()[:, None, :]).sum(2)
    dwdot = (w * dsdot).sum(1, keepdim=True) \
        + (t + 1) * U32 * (w * sdot).abs().sum(1, keepdim=True)
    ds = w * (dsdot + dwdot) + 2 * U32 * w * (sdot.abs() + wdot.abs())
    return {"dscores": torch.where(mask, ds, torch.zeros_like(ds)),
            "dseq": U32 * r["dseq"].abs()}


# ---------------------------------------------------------------- checks

def assert_within(got, ref, bound, what):
    """Every element of got within bound of the fp64 ref; no NaN."""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    err = (got - ref).abs()
    over = err > bound
    if over.any():
        i = tuple(over.nonzero()[0].tolist())
        raise AssertionError(
            f"{what}: {int(over.sum())} of {over.numel()} elements over the "
            f"bound; first at {i}: err {err[i].item():.3e} > "
            f"{bound[i].item():.3e} (got {got[i].item():.8g}, ref "
            f"{ref[i].item():.8g}); worst err/bound "
            f"{float((err / bound.clamp(min=1e-300))[over].max()):.3g}")
