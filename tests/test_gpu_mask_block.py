"""The mask-block kernels (ops/hip/mask_kernels.hip) against fp64 references
on the CPU, operands carved out of NaN-filled buffers so that a read past
an operand shows.

Forward bounds, in the manner of S.resln_fwd_bounds, from the exact
p = bf(m h) the kernel forms in registers (U32, BF, RSQRT_REL of
tests/seq_reference.py, linear_bounds of tests/dense_reference.py):
  v = p W^T + b: K-term fp32 accumulation and the bias add,
      dv <= K U32 (|p| |W|^T) + U32 |v|;  z = bf(v): BF (|v| + dv) + dv
  mean of the N computed v: dmean <= mean(dv) + (N + 1) U32 mean|v|
  d = v - mean: dd <= dv + dmean + U32 |d|
  var = mean(d^2): dvar <= mean(2 |d| dd + dd^2) + (N + 2) U32 var
  rstd: relative rel = 0.5 dvar / (var + eps) + RSQRT_REL + U32
  y = relu(d rstd gamma + beta), relu being 1-Lipschitz, absolute:
      e = |gamma| rstd dd + |d rstd gamma| rel + 3 U32 (|d rstd gamma|
          + |beta|);  dy <= BF (|pre| + e) + e
Backward: S.resln_bwd_bounds as it stands, on g = (y > 0 ? dy : 0), with
the addition-chain depth of k_ln_relu_bwd's launch (min(ceil(M / 32), 1024)
blocks of 4 waves, one row per wave and pass): ceil(M / (4 blocks)) per
lane, 4 waves in LDS, the blocks in global memory.

Model wiring: observed rel_l2 ratios fused / autocast-unfused against the
fp64 model are recorded in profiles/PERF_LOG.md ("Fused mask blocks").
"""
import functools

import pytest
import torch

from tests import dense_reference as D
from tests import seq_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
# (M, N, K): smallest; all ragged, odd K, partial row tile and second wave;
# third wave of 2 columns, K % 32 == 0; full width at the model's K;
# interior path
SHAPES = [(1, 1, 1), (17, 72, 45), (5, 130, 64), (33, 256, 429),
          (16, 256, 256)]
# backward only: the grid-stride loop and the cross-block merge both run
BWD_SHAPES = SHAPES + [(2049, 256, 32)]


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _gpu(*tensors):
    return [D.carve(t, DEV)[0] for t in tensors]


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    gen = S._gen(m, n, k, 19)
    c = {"m": S.randn_bf16(gen, m, k), "h": S.randn_bf16(gen, m, k),
         "w": S.randn_bf16(gen, n, k, scale=k ** -0.5),
         "bias": 0.1 * torch.randn(n, generator=gen),
         "dy": S.randn_bf16(gen, m, n),
         "gamma": S.resln_case(1, n)["gamma"],
         "beta": S.resln_case(1, n)["beta"]}
    c["p"] = (c["m"].float() * c["h"].float()).to(S.BF16)
    return c


def _fwd(c, save=True, variant=-1):
    ops = _gpu(*(c[k] for k in ("m", "h", "w", "bias", "gamma", "beta")))
    return [t.cpu() for t in
            _ext().maskblock_fwd(*ops, EPS, save, variant)]


@functools.lru_cache(maxsize=None)
def _run(m, n, k):
    """(y, z, stats, p) of the default kernel, shared by the tests."""
    return _fwd(_case(m, n, k))


def _fwd_ref(c):
    p, w = c["p"].double(), c["w"].double()
    gamma, beta = c["gamma"].double(), c["beta"].double()
    n, k = w.shape
    v = p @ w.t() + c["bias"].double()
    dv = D.linear_bounds(p, w.t(), v, k)[1] + S.U32 * v.abs()
    mean = v.mean(1, keepdim=True)
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    core = d * rstd * gamma
    dmean = dv.mean(1, keepdim=True) \
        + (n + 1) * S.U32 * v.abs().mean(1, keepdim=True)
    dd = dv + dmean + S.U32 * d.abs()
    dvar = (2 * d.abs() * dd + dd * dd).mean(1, keepdim=True) \
        + (n + 2) * S.U32 * var
    rel = 0.5 * dvar / (var + EPS) + S.RSQRT_REL + S.U32
    e = gamma.abs() * rstd * dd + core.abs() * rel \
        + 3 * S.U32 * (core.abs() + beta.abs())
    ref = {"z": v, "stats": torch.cat([mean, rstd], 1),
           "y": torch.relu(core + beta)}
    bound = {"z": S.BF * (v.abs() + dv) + dv,
             "stats": torch.cat([dmean, rstd * rel], 1),
             "y": S.BF * ((core + beta).abs() + e) + e}
    return ref, bound


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_p_is_exact_and_save_changes_nothing(m, n, k):
    c = _case(m, n, k)
    y, z, stats, p = _run(m, n, k)
    assert torch.equal(p, c["p"])
    assert not torch.isnan(y.float()).any()
    y0, *rest = _fwd(c, save=False)
    assert torch.equal(y0, y)
    assert all(t.numel() == 0 for t in rest)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_z_is_bit_exact_on_integer_operands(m, n, k, variant):
    """Integer h, w and half-integer bias of D.fwd_case, m in {-1, 0, 1}:
    every operand is bf16-exact and every partial sum exact in fp32, so z
    is the int64 result rounded once."""
    fc = D.fwd_case(m, n, k)
    sign = torch.randint(-1, 2, (m, k), generator=S._gen(m, n, k, 23))
    assert all(D.bf16_exact(t.double())
               for t in (sign, fc["x"], fc["w"], fc["bias"]))
    pre = ((sign * fc["x"]) @ fc["w"].t()).double() + fc["bias"].double()
    want = D.to_bf16_rne(pre)
    c = dict(_case(m, n, k), m=sign.to(S.BF16), h=fc["x"].to(S.BF16),
             w=fc["w"].to(S.BF16), bias=fc["bias"])
    assert torch.equal(_fwd(c, variant=variant)[1], want)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_forward_within_derived_bounds(m, n, k, variant):
    c = _case(m, n, k)
    ref, bound = _fwd_ref(c)
    # the default is variant 1 (MT = 2)
    y, z, stats, _ = _run(m, n, k) if variant == 1 else _fwd(c, variant=0)
    for key, got in (("z", z), ("stats", stats), ("y", y)):
        S.assert_within(got, ref[key], bound[key], f"{key} {m, n, k}")


def _bwd_depth(m):
    blocks = min((m + 31) // 32, 1024)
    return -(-m // (4 * blocks)) + 4 + blocks


@pytest.mark.parametrize("m,n,k", BWD_SHAPES)
def test_ln_relu_bwd_within_derived_bounds(m, n, k, monkeypatch):
    c = _case(m, n, k)
    y, z, stats, _ = _run(m, n, k)
    g = torch.where(y.float() > 0, c["dy"], torch.zeros_like(c["dy"]))
    r = S.resln_bwd_ref(g, z, stats, c["gamma"])
    monkeypatch.setattr(S, "resln_bwd_depth", _bwd_depth)
    bound = S.resln_bwd_bounds(r)
    got = _ext().ln_relu_bwd(*_gpu(c["dy"], y, z, stats, c["gamma"]))
    for key, t in zip(("dz", "dgamma", "dbeta"), got):
        S.assert_within(t, r[key], bound[key], f"{key} {m, n, k}")


@pytest.mark.parametrize("m,k", [(17, 45), (1, 7), (300, 429)])
def test_mask_split_bwd_is_exact(m, k):
    gen = S._gen(m, k, 29)
    dp, mk, h = (S.randn_bf16(gen, m, k) for _ in range(3))
    dm, dh = _ext().mask_split_bwd(*_gpu(dp, mk, h))
    assert torch.equal(dm.cpu(), (dp.float() * h.float()).to(S.BF16))
    assert torch.equal(dh.cpu(), (dp.float() * mk.float()).to(S.BF16))


@pytest.mark.parametrize("bad", ["strided", "wide", "mismatch"])
def test_host_checks(bad):
    m, n, k = 16, 257 if bad == "wide" else 8, 16

    def mat(rows, cols, dtype=S.BF16):
        if bad == "strided":
            return torch.zeros(rows, 2 * cols, device=DEV, dtype=dtype)[:, ::2]
        return torch.zeros(rows, cols, device=DEV, dtype=dtype)
    vec = torch.zeros(n, device=DEV)
    other = mat(m + (bad == "mismatch"), k)
    with pytest.raises(RuntimeError, match="maskblock_fwd"):
        _ext().maskblock_fwd(mat(m, k), other, mat(n, k).contiguous(), vec,
                             vec, vec, EPS, True)
    with pytest.raises(RuntimeError, match="mask_split_bwd"):
        _ext().mask_split_bwd(mat(m, n), mat(m + (bad != "strided"), n),
                              mat(m, n))
    other = mat(m + (bad == "mismatch"), n)
    with pytest.raises(RuntimeError, match="ln_relu_bwd"):
        _ext().ln_relu_bwd(mat(m, n), other, mat(m, n),
                           torch.zeros(m, 2, device=DEV), vec)


def _graph_has(fn, name, seen):
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return name in type(fn).__name__ or any(
        _graph_has(nxt, name, seen) for nxt, _ in fn.next_functions)


def test_model_fused_against_autocast(batch=32):
    """Logits and every dense parameter gradient of MaskNet, fused and
    unfused under bf16 autocast, each against the fp64 unfused model on the
    same weights and inputs. The yardstick is autocast's own bf16 noise;
    the fused path also rounds p and the saved z, hence the factor 2.
    The weights are those of seed 0. head.bias is one element, which
    autocast returns as one bf16 value, so its yardstick is mostly the
    distance of the fp64 value to the bf16 grid: it runs from 2.7e-6
    (seed 5, the fp64 value 2.7e-6 away from a grid point) to 6e-3 over
    seeds 0-7 of the reference models alone, while a mean logit error of
    bf16 size puts about 1e-3 on either path.
    Observed on an MI355X (fused / autocast): logits 5.2e-3 / 5.5e-3;
    ratios between 0.35 and 1.14 for every gradient but
    mask_gens.0.0.bias (1.38) and head.bias (0.06); the full list is in
    profiles/PERF_LOG.md, "Fused mask blocks"."""
    from deeprec_amd.models.zoo import MaskNet
    gen = S._gen(batch, 31)
    emb = S.randn_bf16(gen, batch, 26, 4)
    dense = S.randn_bf16(gen, batch, 13).double()
    labels = (torch.rand(batch, generator=gen) < 0.5).double()
    torch.manual_seed(0)
    kw = dict(embedding_dim=4, hidden=32, n_blocks=2)
    models = {"ref": MaskNet(device="cpu", bf16=False, **kw).double(),
              "fused": MaskNet(device=DEV, fused_blocks=True, **kw),
              "autocast": MaskNet(device=DEV, **kw)}
    assert set(models["fused"].state_dict()) == set(
        models["autocast"].state_dict())
    res = {}
    for key, model in models.items():
        with torch.no_grad():
            for q, src in zip(model.parameters(),
                              models["ref"].parameters()):
                q.copy_(src)
        dev = model.device_
        model.sparse_feats = lambda ids, train=True, d=dev: emb.to(d)
        with torch.autocast("cuda", dtype=torch.bfloat16,
                            enabled=key == "autocast"):
            logits = model(dense.to(dev, next(model.parameters()).dtype),
                           None)
        assert _graph_has(logits.grad_fn, "_MaskBlock", set()) == (
            key == "fused")
        torch.nn.functional.binary_cross_entropy_with_logits(
            logits.double(), labels.to(dev)).backward()
        res[key] = {name: q.grad.detach().cpu().double()
                    for name, q in model.named_parameters()}
        res[key]["logits"] = logits.detach().cpu().double()
    for what, ref in res["ref"].items():
        fused = S.rel_l2(res["fused"][what], ref)
        plain = S.rel_l2(res["autocast"][what], ref)
        print(f"masknet {what}: fused {fused:.3e} autocast {plain:.3e} "
              f"ratio {fused / plain:.2f}")
        assert fused <= 2 * plain, what
