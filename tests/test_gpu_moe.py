"""The grouped-expert kernels (ops/hip/moe_kernels.hip) and the fused expert
block of MMoE / PLE against the contract of docs/KERNELS.md.

Bit for bit: every expert slab of expert_fwd and of expert_mix_fwd's ex
against linear_fwd, the mixture where its value is exact, expert_dx on the
exact-integer operands of tests/dense_reference.py. Everything else against
fp64 formulas with bounds derived below; the softmax and its backward are
those of the masked softmax pool, so tests/seq_reference.py's references
and bounds are used as they are, with (sample, task) as the row, the expert
as the position and H as the width.

Observed on an MI355X (test_model_fused_against_unfused): fused error /
unfused error between 0.99 and 1.01 for every group of both models; the
figures are in profiles/PERF_LOG.md.
"""
import functools

import pytest
import torch

from deeprec_amd.models.zoo import MMoE, PLE
from tests import dense_reference as D
from tests import seq_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U32 = S.U32
PLE_MASK = [[1, 1, 1, 1, 0, 0], [1, 1, 0, 0, 1, 1]]


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _dev(values):
    """On the GPU inside a NaN-filled buffer: a read past the operand
    shows."""
    return D.carve(values.contiguous(), DEV)[0]


def _mask(rows):
    return torch.tensor(rows, dtype=torch.uint8)


# ------------------------------------------------- forward, per expert slab

@pytest.mark.parametrize("shared", [True, False], ids=["shared", "stacked"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 17, 72, 45),
                                   (2, 80, 130, 429)], ids=str)
def test_expert_slabs_equal_linear_fwd(shape, act, shared):
    e, b, n, k = shape
    gen = S._gen(e, b, n, k)
    a = _dev(S.randn_bf16(gen, *((b, k) if shared else (e, b, k))))
    w = _dev(S.randn_bf16(gen, e, n, k, scale=k ** -0.5))
    bias = _dev(torch.randn(e, n, generator=gen))
    ext = _ext()
    out = ext.expert_fwd(a, w, bias, act)
    gate = torch.zeros(b, 1, e, device=DEV)
    _, ex, _ = ext.expert_mix_fwd(a, w, bias, act, gate,
                                  _mask([[1] * e]), True)
    for i in range(e):
        want = ext.linear_fwd(a if shared else a[i], w[i], bias[i], act)
        assert torch.equal(out[i], want), f"expert_fwd slab {i}"
        assert torch.equal(ex[i], want), f"expert_mix_fwd ex slab {i}"


# ------------------------------------------------ mixture, exact structure

def test_one_expert_per_task_is_that_expert():
    gen = S._gen(3, 17, 72, 45)
    a, w = S.randn_bf16(gen, 17, 45), S.randn_bf16(gen, 3, 72, 45, scale=.15)
    gate = torch.randn(17, 2, 3, generator=gen)
    mix, ex, p = _ext().expert_mix_fwd(
        _dev(a), _dev(w), _dev(torch.randn(3, 72, generator=gen)), 0,
        _dev(gate), _mask([[0, 0, 1], [1, 0, 0]]), True)
    assert torch.equal(mix[0], ex[2]) and torch.equal(mix[1], ex[0])
    assert torch.equal(p.cpu(), torch.tensor([[0., 0, 1], [1, 0, 0]])
                       .expand(17, 2, 3))


def test_quarter_weights_are_exact_and_a_masked_nan_stays_out():
    """Four experts at equal logits: p = 0.25 each. Integer operands scaled
    by 4 make 0.25 * sum_e ex_e a multiple of 0.5 below 128, exact in bf16
    (asserted here, not tried on the GPU). A fifth expert with a NaN bias
    belongs to task 1 alone."""
    b, h = 17, 72
    c = D.fwd_case(b, 4 * h, 1)
    w = 4 * c["w"].view(4, h, 1)
    bias = 4 * c["bias"].view(4, h)
    ex = c["x"].double() @ w.double().transpose(1, 2) + bias.double()[:, None]
    want = 0.25 * ex.sum(0)
    assert D.bf16_exact(ex) and D.bf16_exact(want)
    w5 = torch.cat([w, w[:1]]).to(BF16)
    bias5 = torch.cat([bias, torch.full((1, h), float("nan"))])
    mix, _, _ = _ext().expert_mix_fwd(
        _dev(c["x"].to(BF16)), _dev(w5), _dev(bias5), 0,
        torch.full((b, 2, 5), 1.5, device=DEV),
        _mask([[1, 1, 1, 1, 0], [0, 0, 0, 0, 1]]), False)
    assert torch.equal(mix[0].cpu(), want.to(BF16))
    assert torch.isnan(mix[1].float()).all()


# ------------------------------------------------------- mixture, general

MIX_SHAPES = [(3, 2, 17, 72, 45), (6, 2, 33, 130, 64), (16, 4, 16, 16, 32)]


@functools.lru_cache(maxsize=None)
def mix_run(shape):
    """One forward and two backward runs of a case, results on the CPU."""
    e, t, b, h, k = shape
    gen = S._gen(*shape)
    if e == 6:
        mask = _mask(PLE_MASK)
    else:
        mask = (torch.rand(t, e, generator=gen) < 0.6).to(torch.uint8)
        mask[torch.arange(t), torch.randint(0, e, (t,), generator=gen)] = 1
    c = {"mask": mask, "gate": torch.randn(b, t, e, generator=gen) * 2,
         "dmix": S.randn_bf16(gen, t, b, h)}
    ext = _ext()
    out = ext.expert_mix_fwd(
        _dev(S.randn_bf16(gen, b, k)),
        _dev(S.randn_bf16(gen, e, h, k, scale=k ** -0.5)),
        _dev(torch.randn(e, h, generator=gen)), 1, _dev(c["gate"]), mask,
        True)
    bwd = [ext.expert_mix_bwd(_dev(c["dmix"]), out[2], out[1], mask, 1)
           for _ in range(2)]
    c.update(zip(("mix", "ex", "p"), (v.cpu() for v in out)))
    c["bwd"] = [tuple(v.cpu() for v in r) for r in bwd]
    # the softmax-pool view: row (b, t), position e, width h
    c["live"] = mask.bool()[None].expand(b, t, e).reshape(b * t, e)
    c["seq"] = c["ex"].double().permute(1, 0, 2)[:, None].expand(
        b, t, e, h).reshape(b * t, e, h)
    return c


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=str)
def test_mixture_forward(shape):
    e, t, b, h, _ = shape
    c = mix_run(shape)
    r = S.msm_fwd_ref(c["gate"].reshape(b * t, e), c["seq"], c["live"])
    assert S.exp_precondition(r["arg"], c["live"])
    dp = S.msm_fwd_bounds(r, c["seq"], c["live"])["w"]
    S.assert_within(c["p"].reshape(b * t, e), r["w"], dp, "p")
    assert (c["p"].reshape(b * t, e)[~c["live"]] == 0).all()
    # mix = bf(s), s the fp32 fma chain over p_hat = p + dp:
    #   |s - ref| <= d = sum_e dp_e |ex_e| + E U32 sum_e (p_e + dp_e) |ex_e|
    # and bf(s) is the grid point nearest s, the one nearest ref is within
    # half an ulp of ref: |bf(s) - ref| <= ulp(ref) / 2 + 2 d
    ref = r["out"].reshape(b, t, h).transpose(0, 1)
    sabs = c["seq"].abs()
    d = (dp[:, :, None] * sabs).sum(1) + e * U32 * (
        (r["w"] + dp)[:, :, None] * sabs).sum(1)
    bound = 0.5 * S.bf16_ulp(ref) + 2 * d.reshape(b, t, h).transpose(0, 1)
    S.assert_within(c["mix"], ref, bound, "mix")


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=str)
def test_mixture_backward(shape):
    e, t, b, h, _ = shape
    c = mix_run(shape)
    (dex, dgate), again = c["bwd"]
    assert torch.equal(dex, again[0]) and torch.equal(
        dgate.view(torch.int32), again[1].view(torch.int32))
    live3 = c["live"].reshape(b, t, e)
    p = torch.where(live3, c["p"].double(), torch.zeros((), dtype=F64))
    dm = c["dmix"].double()
    # dpre: a T-term fp32 fma chain, one bf16 rounding, then the relu rule
    terms = p.permute(2, 1, 0)[..., None] * dm[None]          # [E,T,B,H]
    on = c["ex"] > 0
    ref = torch.where(on, terms.sum(1), torch.zeros((), dtype=F64))
    bound = 0.5 * S.bf16_ulp(ref) + 2 * t * U32 * terms.abs().sum(1)
    S.assert_within(dex, ref, bound, "dex")
    assert (dex[~on] == 0).all()
    r = S.msm_bwd_ref(dm.transpose(0, 1).reshape(b * t, h), c["seq"],
                      c["p"].reshape(b * t, e), c["live"])
    S.assert_within(dgate.reshape(b * t, e), r["dscores"],
                    S.msm_bwd_bounds(r, c["live"])["dscores"], "dgate")
    assert (dgate[~live3] == 0).all()


# ------------------------------------------------------------- expert_dx

@pytest.mark.parametrize("n", [127, 130])
def test_expert_dx_exact(n, e=3, m=17, k=45):
    cases = [D.dx_case(m + i, n, k) for i in range(e)]
    g = torch.stack([c["g"][:m] for c in cases])
    w = torch.stack([c["w"] for c in cases])
    ref = (g @ w).double()
    assert float(ref.abs().sum(0).max()) < D.EXACT_LIMIT
    prev = D.int_matrix(e * m, k, (-2, 2), n).view(e, m, k)
    ext, g16, w16 = _ext(), _dev(g.to(BF16)), _dev(w.to(BF16))
    assert torch.equal(ext.expert_dx(g16, w16).cpu(), D.to_bf16_rne(ref))
    fused = ext.expert_dx(g16, w16, _dev(prev.to(BF16)), 1)
    assert torch.equal(fused.cpu(), torch.where(
        prev > 0, D.to_bf16_rne(ref), torch.zeros((), dtype=BF16)))
    assert torch.equal(ext.expert_dx(g16, w16, reduce=True).cpu(),
                       D.to_bf16_rne(ref.sum(0)))


def test_expert_dx_reduce_random(e=3, m=33, n=130, k=72):
    gen = S._gen(e, m, n, k)
    g, w = S.randn_bf16(gen, e, m, n), S.randn_bf16(gen, e, n, k, scale=.1)
    a = g.double().transpose(0, 1).reshape(m, e * n)
    bmat = w.double().reshape(e * n, k)
    bound, _ = D.linear_bounds(a, bmat, a @ bmat, e * n)
    got = _ext().expert_dx(_dev(g), _dev(w), reduce=True)
    S.assert_within(got, a @ bmat, bound, "dx reduce")


# ------------------------------------------------------------ model level

def _graph_has(fn, name, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return name in type(fn).__name__ or any(
        _graph_has(nxt, name, seen) for nxt, _ in fn.next_functions)


@pytest.mark.parametrize("cls", [MMoE, PLE])
def test_model_fused_against_unfused(cls, batch=32):
    """Logits and parameter gradients of one backward, flag on and off,
    each against the fp32 CPU model on the same weights and inputs: both
    are bf16 pipelines that differ in the mixture's summation and one
    rounding, so the fused error may be at most twice the unfused one —
    for the logits and for the gradients of the experts, the gates and the
    towers, each group taken as one vector."""
    gen = S._gen(batch, 7)
    emb = S.randn_bf16(gen, batch, 26, 4)
    dense = S.randn_bf16(gen, batch, 13).float()
    labels = (torch.rand(batch, generator=gen) < 0.5).float()
    torch.manual_seed(3)
    kw = dict(embedding_dim=4, expert_sizes=(32, 16))
    models = {"ref": cls(device="cpu", bf16=False, **kw),
              "plain": cls(device=DEV, **kw),
              "fused": cls(device=DEV, fused_experts=True, **kw)}
    res = {}
    for key, m in models.items():
        with torch.no_grad():   # same parameter order whatever the layers
            for q, src in zip(m.parameters(), models["ref"].parameters()):
                q.copy_(src)
        dev = m.device_
        m.sparse_feats = lambda ids, train=True, d=dev, m=m: emb.to(
            d, m.compute_dtype)
        logits = m(dense.to(dev), None)
        assert _graph_has(logits[0].grad_fn, "_ExpertMixture") == (
            key == "fused")
        m.loss_fn(logits, labels.to(dev)).backward()
        grads = {"experts": [], "gates": [], "towers": []}
        for name, q in m.named_parameters():
            group = "experts" if name.split(".")[0] in (
                "experts", "shared", "spec") else name.split(".")[0]
            grads[group].append(q.grad.detach().cpu().double().flatten())
        res[key] = {g: torch.cat(v) for g, v in grads.items()}
        res[key]["logits"] = torch.cat(
            [lg.detach().cpu().double() for lg in logits])
    for what, ref in res["ref"].items():
        fused = S.rel_l2(res["fused"][what], ref)
        plain = S.rel_l2(res["plain"][what], ref)
        print(f"{cls.__name__} {what}: fused {fused:.3e} unfused "
              f"{plain:.3e} ratio {fused / plain:.2f}")
        assert fused <= 2 * plain, what
