"""The sequence-kernel references proven without a GPU.

tests/test_gpu_seq_kernels.py compares the HIP kernels with the fp64
references of tests/seq_reference.py inside bounds derived there. That is
only sound if the references are right and the bounds are neither wrong
nor vacuous; this file shows, for every case of the tables:
  * the fp64 forwards equal torch's own ops (nn.GRU, layer_norm, normalize,
    softmax attention) to rtol 1e-12;
  * the explicit backward formulas equal fp64 autograd of those forwards
    when nothing is rounded;
  * what rounding the gates, dpre and h_prev to bf16 costs (the "storage
    noise" the end-to-end GPU test scales its limit by);
  * the same references evaluated in fp32 on the CPU stay inside their own
    bounds, the exp-argument precondition holds, and the fp32 reference
    flips at most a quarter of the allowed share of bf16 outputs.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import seq_reference as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
TIGHT = dict(rtol=1e-12, atol=1e-13)
MHA_ALL = [(s, p) for s in R.MHA_SHAPES for p in R.MHA_PADS]
GRU_ALL = [(s, a) for s in R.GRU_SHAPES for a in (False, True)]
CPU_RESLN = R.RESLN_SHAPES


def _ids(cases):
    return ["-".join(str(x) for x in (c if isinstance(c, tuple) else (c,)))
            .replace("(", "").replace(")", "").replace(", ", "x")
            for c in cases]


# -------------------------------------------------------------- attention

def _plain_attention(q, k, v, pad, h, scale):
    b, t, d = q.shape
    dh = d // h
    qs = q.view(b, t, h, dh).transpose(1, 2)
    ks = k.view(b, t, h, dh).transpose(1, 2)
    vs = v.view(b, t, h, dh).transpose(1, 2)
    s = qs @ ks.transpose(-1, -2) * scale
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ vs).transpose(1, 2).reshape(b, t, d)


@pytest.mark.parametrize("shape,pattern", MHA_ALL, ids=_ids(MHA_ALL))
def test_mha_reference(shape, pattern):
    b, t, d, h = shape
    c = R.mha_case(*shape)
    pad = R.mha_pad(b, t, pattern)
    dead = pad.all(1)
    assert bool(dead.any()) == (pattern == "dead")
    if pattern == "last":
        assert bool((~pad).sum(1).eq(1).all()) and not bool(pad[:, -1].any())
    r = R.mha_ref(c["q"], c["k"], c["v"], pad, h, c["scale"], c["dout"])
    assert R.exp_precondition(r["arg"], r["live"])
    leaves = [c[n].double().requires_grad_(True) for n in "qkv"]
    keep = ~dead
    out = _plain_attention(*[x[keep] for x in leaves], pad[keep], h,
                           c["scale"])
    torch.testing.assert_close(r["out"][keep], out.detach(), **TIGHT)
    (out * c["dout"].double()[keep]).sum().backward()
    for name, leaf in zip(("dq", "dk", "dv"), leaves):
        torch.testing.assert_close(r[name], leaf.grad, **TIGHT)
        assert not bool(r[name][dead].any())
    assert not bool(r["out"][dead].any())
    assert bool((r["stats"][dead][..., 0] == R.MHA_DEAD_MAX).all())
    assert bool((r["stats"][dead][..., 1] == 0).all())
    # padded keys receive nothing
    assert not bool(r["dk"][pad].any()) and not bool(r["dv"][pad].any())

    bound = R.mha_bounds(r, c["scale"])
    r32 = R.mha_ref(c["q"], c["k"], c["v"], pad, h, c["scale"], c["dout"],
                    dtype=F32)
    for name in ("out", "dq", "dk", "dv"):
        R.assert_within(r32[name].to(BF16), r[name], bound[name],
                        f"fp32 {name}")
        _, share = R.ulp_flips(r32[name].to(BF16), r[name])
        assert share <= 0.05     # sanity: the fp32 run is the same function
    R.assert_within(r32["stats"][..., 0], r["stats"][..., 0], bound["mx"],
                    "fp32 max")
    R.assert_within(r32["stats"][..., 1], r["stats"][..., 1], bound["sum"],
                    "fp32 sum")
    # the bounds are tight enough to mean something: a probability mass
    # moved by 1 % is far outside
    assert float((bound["out"] - R.BF * r["out"].abs()).max()) < 1e-3


# -------------------------------------------------------------------- GRU

@pytest.mark.parametrize("shape", R.GRU_SHAPES, ids=_ids(R.GRU_SHAPES))
def test_gru_forward_equals_torch_gru(shape):
    b, t, h = shape
    c = R.gru_case(b, t, h, False)
    gru = torch.nn.GRU(R.GRU_IN, h, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(c["w_ih"].double())
        gru.weight_hh_l0.copy_(c["U"].double())
        gru.bias_ih_l0.copy_(c["b_ih"].double())
        gru.bias_hh_l0.copy_(c["bh"].double())
        want, _ = gru(c["x"].double())
    x3 = c["x"].double() @ c["w_ih"].double().t() + c["b_ih"].double()
    got, gates = R.gru_fwd_ref(x3, c["U"], c["bh"], None)
    torch.testing.assert_close(got, want, **TIGHT)
    assert gates.shape == (b, t, 3 * h)
    # X3 as the kernel gets it is that projection rounded once
    assert torch.equal(c["X3"], x3.float().to(BF16))


@pytest.mark.parametrize("shape,augru", GRU_ALL, ids=_ids(GRU_ALL))
def test_gru_backward_formulas(shape, augru):
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    h_ref, ref = R.gru_autograd(c)
    h_out, gates = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    torch.testing.assert_close(h_out, h_ref, **TIGHT)
    exact = R.gru_chain(c, rounded=False)
    assert set(exact) == set(ref)
    for k in ref:
        torch.testing.assert_close(exact[k], ref[k], rtol=1e-10, atol=1e-12,
                                   msg=lambda s, k=k: f"{k}: {s}")

    # storage noise: what the bf16 gates / dpre / h_prev cost
    noise = R.gru_storage_noise(b, t, h, augru)
    print(f"storage noise {shape} augru={augru}: "
          + ", ".join(f"{k}={v:.2e}" for k, v in noise.items()))
    for k, v in noise.items():
        # a few bf16 roundings; the tiny cases have little to average over
        assert math.isfinite(v) and v <= 0.25, (k, v)
        if float(ref[k].norm()) > 0:
            assert v > 0, k
    if t == 1:
        assert float(ref["w_hh"].norm()) == 0      # h_prev is all zero

    # the kernel-level backward, as gru_bwd is fed: fp32 h_out, bf16 gates
    g16 = gates.float().to(BF16)
    h32 = h_out.float()
    dpx, dph, da, da_b = R.gru_bwd_ref(c["dh_out"], h32, g16, c["U"],
                                       c["bh"], c["alpha"], with_bounds=True)
    x32, h32b, a32 = R.gru_bwd_ref(c["dh_out"], h32, g16, c["U"], c["bh"],
                                   c["alpha"], dtype=F32)
    for name, got, want in (("dpre_x", x32, dpx), ("dpre_h", h32b, dph)):
        n_ulp, share = R.ulp_flips(got.to(BF16), want)
        assert n_ulp <= 1 and share <= R.FLIP_CAP / 4, (name, n_ulp, share)
    if augru:
        R.assert_within(a32, da, da_b, "fp32 dalpha")
        # the last step has no carried error; further back the bound grows
        # with the absolute values of the recurrence's coefficients, and
        # stays well below the 8e-2 the fp32-reference test had to allow
        assert float(da_b[:, -1].max()) < 1e-4
        assert float(da_b.max()) < 2e-2
    else:
        assert da is None and a32 is None
    # gates of the fp32 forward: the same flip rule
    _, g32 = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"], dtype=F32)
    n_ulp, share = R.ulp_flips(g32.to(BF16), gates)
    assert n_ulp <= 1 and share <= R.FLIP_CAP / 4, (n_ulp, share)


def test_gru_case_table_reaches_the_paths():
    hs = [s[2] for s in R.GRU_SHAPES]
    assert 21 in hs and 22 in hs and 3 * 21 < 64 < 3 * 22
    assert max(hs) == 32 and min(hs) == 1
    assert any(s[1] == 1 for s in R.GRU_SHAPES)
    assert any(s[0] % 4 for s in R.GRU_SHAPES)


# ------------------------------------------------------ residual LayerNorm

@pytest.mark.parametrize("m,n", CPU_RESLN, ids=_ids(CPU_RESLN))
def test_resln_reference(m, n):
    c = R.resln_case(m, n)
    r = R.resln_fwd_ref(c["x"], c["a"], c["gamma"], c["beta"])
    zl = (c["x"].double() + c["a"].double()).requires_grad_(True)
    gl = c["gamma"].double().requires_grad_(True)
    bl = c["beta"].double().requires_grad_(True)
    want = F.layer_norm(zl, (n,), gl, bl, R.RESLN_EPS)
    torch.testing.assert_close(r["y"], want.detach(), **TIGHT)
    want.backward(c["dy"].double())
    b = R.resln_bwd_ref(c["dy"], r["z"], r["stats"], c["gamma"])
    torch.testing.assert_close(b["dz"], zl.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dgamma"], gl.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(b["dbeta"], bl.grad, rtol=1e-10, atol=1e-11)

    fb = R.resln_fwd_bounds(r, c["gamma"], c["beta"])
    r32 = R.resln_fwd_ref(c["x"], c["a"], c["gamma"], c["beta"], dtype=F32)
    R.assert_within(r32["y"].to(BF16), r["y"], fb["y"], "fp32 y")
    R.assert_within(r32["z"].to(BF16), r["z"], fb["z"], "fp32 z")
    R.assert_within(r32["stats"], r["stats"], fb["stats"], "fp32 stats")
    # backward as the kernel is fed: bf16 z, fp32 stats
    z16, st32 = r["z"].float().to(BF16), r["stats"].float()
    b = R.resln_bwd_ref(c["dy"], z16, st32, c["gamma"])
    bb = R.resln_bwd_bounds(b)
    b32 = R.resln_bwd_ref(c["dy"], z16, st32, c["gamma"], dtype=F32)
    R.assert_within(b32["dz"].to(BF16), b["dz"], bb["dz"], "fp32 dz")
    R.assert_within(b32["dgamma"], b["dgamma"], bb["dgamma"], "fp32 dgamma")
    R.assert_within(b32["dbeta"], b["dbeta"], bb["dbeta"], "fp32 dbeta")
    # relative to what is summed the bound is depth * 2**-23 — nowhere
    # near the atol of 5e-1 the fp32-reference test had to allow
    assert float((bb["dbeta"] / b["g"].abs().sum(0)).max()) < 1e-4
    assert float((bb["dgamma"] / (b["g"] * b["xh"]).abs().sum(0)).max()) < 1e-4
    if m <= 257:
        assert float(bb["dgamma"].max()) < 1e-2


def test_resln_strides_are_reached():
    assert R.RESLN_BWD_STRIDE_M > 64 * 256
    assert R.RESLN_FWD_STRIDE_M > 4096 * 256
    assert R.resln_bwd_depth(R.RESLN_BWD_STRIDE_M) == 2 + 256 + 64
    assert R.resln_bwd_depth(1) == 1 + 256 + 64
    assert (R.RESLN_FWD_STRIDE_M, 16) in R.RESLN_SHAPES


# ---------------------------------------------------------------- l2norm

@pytest.mark.parametrize("m,n", R.L2NORM_SHAPES, ids=_ids(R.L2NORM_SHAPES))
def test_l2norm_reference(m, n):
    c = R.l2norm_case(m, n)
    zero = ~c["x"].float().abs().sum(1).bool()
    assert bool(zero.any()) == (m >= 5)
    r = R.l2norm_fwd_ref(c["x"])
    xl = c["x"].double().requires_grad_(True)
    want = F.normalize(xl, dim=1, eps=math.sqrt(R.L2NORM_EPS))
    torch.testing.assert_close(r["y"], want.detach(), **TIGHT)
    want.backward(c["dy"].double())
    b = R.l2norm_bwd_ref(c["dy"], r["y"], r["inv"])
    torch.testing.assert_close(b["dx"], xl.grad, rtol=1e-10, atol=1e-12)

    fb = R.l2norm_fwd_bounds(r)
    r32 = R.l2norm_fwd_ref(c["x"], dtype=F32)
    R.assert_within(r32["y"].to(BF16), r["y"], fb["y"], "fp32 y")
    R.assert_within(r32["inv"], r["inv"], fb["inv"], "fp32 inv")
    y16, inv32 = r["y"].float().to(BF16), r["inv"].float()
    b = R.l2norm_bwd_ref(c["dy"], y16, inv32)
    b32 = R.l2norm_bwd_ref(c["dy"], y16, inv32, dtype=F32)
    R.assert_within(b32["dx"].to(BF16), b["dx"], R.l2norm_bwd_bounds(b)["dx"],
                    "fp32 dx")


# -------------------------------------------------------------- din_feat

@pytest.mark.parametrize("b,t,d", R.DIN_SHAPES, ids=_ids(R.DIN_SHAPES))
def test_din_case_is_exact(b, t, d):
    c = R.din_case(b, t, d)
    for k in ("seq", "tgt", "g"):
        assert int(c[k].abs().max()) <= R.DIN_RANGE
    for k in ("out", "dseq", "dtgt"):
        assert int(c[k].abs().max()) < 2 ** 24
    # every forward output is on the bf16 grid
    assert torch.equal(c["out"].double().to(BF16).double(), c["out"].double())
    assert int(c["out"].abs().max()) <= R.DIN_RANGE ** 2
    # the floating-point form holds the same values, plus the sign of zero
    assert torch.equal(c["out_f"], c["out"].double())
    if b * t * d > 1000:
        assert bool(torch.signbit(c["out_f"][c["out_f"] == 0]).any())
    # autograd of the torch formula agrees
    s = c["seq"].double().requires_grad_(True)
    tg = c["tgt"].double().requires_grad_(True)
    te = tg[:, None, :].expand(b, t, d)
    out = torch.cat([s, te, s - te, s * te], 2).reshape(b * t, 4 * d)
    assert torch.equal(out.detach(), c["out"].double())
    out.backward(c["g"].double())
    assert torch.equal(s.grad, c["dseq"].double())
    assert torch.equal(tg.grad, c["dtgt"].double())
    if (b, t, d) == R.DIN_SHAPES[-1]:
        assert b * t * d > 8192 * 256


# -------------------------------------------------------------- msm_pool

@pytest.mark.parametrize("b,t,d", R.MSM_SHAPES, ids=_ids(R.MSM_SHAPES))
def test_msm_reference(b, t, d):
    c = R.msm_case(b, t, d)
    r = R.msm_fwd_ref(c["scores"], c["seq"], c["mask"])
    assert R.exp_precondition(r["arg"], c["mask"])
    sl = c["scores"].double().requires_grad_(True)
    ql = c["seq"].double().requires_grad_(True)
    w = torch.softmax(sl.masked_fill(~c["mask"], float("-inf")), 1)
    out = (w[:, :, None] * ql).sum(1)
    torch.testing.assert_close(r["out"], out.detach(), **TIGHT)
    torch.testing.assert_close(r["w"], w.detach(), **TIGHT)
    out.backward(c["dout"].double())
    bw = R.msm_bwd_ref(c["dout"], c["seq"], r["w"], c["mask"])
    torch.testing.assert_close(bw["dscores"], sl.grad, rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(bw["dseq"], ql.grad, rtol=1e-10, atol=1e-13)

    fb = R.msm_fwd_bounds(r, c["seq"], c["mask"])
    r32 = R.msm_fwd_ref(c["scores"], c["seq"], c["mask"], dtype=F32)
    R.assert_within(r32["w"], r["w"], fb["w"], "fp32 w")
    R.assert_within(r32["out"], r["out"], fb["out"], "fp32 out")
    w32 = r["w"].float()
    bw = R.msm_bwd_ref(c["dout"], c["seq"], w32, c["mask"])
    bb = R.msm_bwd_bounds(bw, c["mask"])
    b32 = R.msm_bwd_ref(c["dout"], c["seq"], w32, c["mask"], dtype=F32)
    R.assert_within(b32["dscores"], bw["dscores"], bb["dscores"],
                    "fp32 dscores")
    R.assert_within(b32["dseq"], bw["dseq"], bb["dseq"], "fp32 dseq")


# ------------------------------------------------------------ small tools

def test_ulp_flips_and_rel_l2():
    ref = torch.tensor([1.0, 2.0, 3.0, 1.0 + 2.0 ** -7], dtype=F64)
    same = ref.float().to(BF16)
    assert R.ulp_flips(same, ref) == (0.0, 0.0)
    off = same.clone()
    off[1] = 2.0 + 2.0 ** -6                  # next bf16 above 2
    n_ulp, share = R.ulp_flips(off, ref)
    assert n_ulp == 1.0 and share == 0.25
    off[1] = 2.0 + 2.0 ** -5
    assert R.ulp_flips(off, ref)[0] == 2.0
    # across a binade: 1 - 2**-8 is one step below 1
    assert R.ulp_flips(torch.tensor([1 - 2.0 ** -8]).to(BF16),
                       torch.tensor([1.0], dtype=F64))[0] <= 1.0
    assert R.rel_l2(torch.zeros(3), torch.zeros(3)) == 0.0
    assert R.rel_l2(torch.ones(3), torch.zeros(3)) == float("inf")
    assert abs(R.rel_l2(torch.tensor([1.0, 1.0]), torch.tensor([1.0, 0.0]))
               - 1.0) < 1e-15


def test_assert_within_reports():
    ref = torch.zeros(2, 2, dtype=F64)
    R.assert_within(torch.zeros(2, 2), ref, torch.full((2, 2), 1e-3), "ok")
    with pytest.raises(AssertionError, match="1 of 4"):
        got = torch.zeros(2, 2)
        got[1, 0] = 1.0
        R.assert_within(got, ref, torch.full((2, 2), 1e-3, dtype=F64), "x")
    with pytest.raises(AssertionError, match="NaN"):
        R.assert_within(torch.full((2, 2), float("nan")), ref,
                        torch.ones(2, 2, dtype=F64), "x")


# ------------------------------------------- CPU paths of the python ops

def test_torch_mha_fully_padded_sample_is_zero_and_passes_no_gradient():
    from deeprec_amd.ops.fused_attention import _torch_mha
    b, t, d, h = 2, 17, 16, 4
    c = R.mha_case(b, t, d, h)
    pad = R.mha_pad(b, t, "dead")
    q, k, v = (c[n].float().requires_grad_(True) for n in "qkv")
    out = _torch_mha(q, k, v, pad, h, c["scale"])
    assert not bool(out[0].any())
    r = R.mha_ref(c["q"], c["k"], c["v"], pad, h, c["scale"], c["dout"])
    torch.testing.assert_close(out.double(), r["out"], rtol=1e-5, atol=1e-6)
    out.backward(c["dout"].float())
    for name, leaf in (("dq", q), ("dk", k), ("dv", v)):
        assert not bool(leaf.grad[0].any()), name
        assert bool(torch.isfinite(leaf.grad).all())
        torch.testing.assert_close(leaf.grad.double(), r[name], rtol=1e-4,
                                   atol=1e-5)


def test_din_attend_cpu_empty_history_pools_to_zero():
    """DIN.attend's CPU branch follows masked_softmax_pool's rule: a user
    with no history pools to zeros (and trains nothing), as on the GPU."""
    from deeprec_amd.models.sequence import DIN
    from deeprec_amd.ops.fused_attention import masked_softmax_pool
    torch.manual_seed(3)
    m = DIN(device="cpu", bf16=False)
    b, t = 4, 6
    d = m.item_dim
    seq = torch.randn(b, t, d, requires_grad=True)
    tgt = torch.randn(b, d)
    mask = torch.rand(b, t) > 0.4
    mask[:, 0] = True
    mask[1] = False
    out = m.attend(seq, tgt, mask)
    assert out.shape == (b, d) and not bool(out[1].any())
    out.sum().backward()
    assert not bool(seq.grad[1].any())
    # live rows: the softmax over the valid positions
    te = tgt.unsqueeze(1).expand_as(seq)
    scores = m.att(torch.cat([seq, te, seq - te, seq * te], 2)).squeeze(2)
    w = torch.softmax(scores.masked_fill(~mask, float("-inf")), 1)
    want = (w.unsqueeze(2) * seq).sum(1)
    live = mask.any(1)
    torch.testing.assert_close(out[live], want[live].detach(), rtol=1e-5,
                               atol=1e-6)
    # masked_softmax_pool's CPU path ignores the scores of masked slots
    s2 = scores.detach().clone()
    s2[~mask] = 1e4
    torch.testing.assert_close(masked_softmax_pool(s2, seq.detach(), mask),
                               out.detach(), rtol=1e-5, atol=1e-6)
