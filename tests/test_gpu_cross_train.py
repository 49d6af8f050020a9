"""The training kernels of the DCNv2 cross stack (ops/hip/cross_kernels.hip:
cross_lr_bwd, cross_du, cross_dx; the low-rank forward is linear_fwd +
cross_fwd, a one-launch forward having measured no faster) and the
cross_stack autograd node against the numerical contract of docs/KERNELS.md.

Kernels, bit for bit: small integer operands (biases multiples of 0.5) keep
every intermediate below 2**23, exact in fp32 in any summation order, so an
int64 reference with the contract's bf16 roundings has to match every output
exactly. V and the backward's operands are wide enough that at D = 429 a fair
share of t and dt really rounds. Every operand is a view inside a NaN-filled
buffer.

Node: each gradient's relative L2 error against fp64 autograd of the plain
formula, between E2E_NOISE_FLOOR and E2E_NOISE_FACTOR times its storage
noise: the distance between the explicit fp64 forward/backward with the
contract's roundings and the same function without them, which itself has to
equal autograd to 1e-12. x0 and the weights are bf16-representable.

Observed on an MI355X: error / storage noise 1.00 for every gradient (x0,
weights, biases) of all four cases.
"""
import functools

import pytest
import torch

from deeprec_amd.models.zoo import DCN, MLPerfDLRMDCN, _CrossNet
from tests import dense_reference as D
from tests.seq_reference import randn_bf16, rel_l2, _gen
from tests.test_gpu_cross import (DEV, BF16, E2E_NOISE_FACTOR,
                                  E2E_NOISE_FLOOR, EXACT_LIMIT,
                                  _assert_bits_equal, _dev, _ext)

pytestmark = pytest.mark.gpu

LR_SHAPES = [(1, 1, 1), (17, 45, 5), (80, 429, 32), (33, 100, 72),
             (20, 130, 128)]
FULL_SHAPES = [(1, 1), (17, 45), (80, 429)]
E2E_CASES = [(45, 0), (429, 0), (45, 5), (429, 32)]
NARROW, WIDE = (-4, 4), (-7, 7)


@functools.lru_cache(maxsize=None)
def int_case(b, d, r):
    """Operands and exact results of one layer, forward and backward; r = 0
    is the full-matrix layer (backward only)."""
    seed = 9000011 * b + 9001 * d + 17 * r
    mat = lambda i, rows, cols, rng=NARROW: D.int_matrix(  # noqa: E731
        rows, cols, rng, seed + i)
    c = {k: mat(i, b, d) for i, k in enumerate(
        ("a", "x", "x0", "g", "us", "dx0"))}
    c["bias"] = D.half_bias(d, seed + 9)
    exact, du = [], c["g"] * c["x0"]
    # the product as floating point: -1 * 0 is -0 there and in the kernel
    c["du16"] = D.to_bf16_rne(c["g"].double() * c["x0"].double())
    c["dx0n"] = (c["dx0"] + c["g"] * c["us"]).float()
    if r == 0:
        c["w"] = mat(6, d, d, WIDE)
        gp = c["g"] + du @ c["w"]
    else:
        c["v"], c["u"] = mat(7, r, d, WIDE), mat(8, d, r)
        t = (c["a"] @ c["v"].t()).double()
        c["t16"] = D.to_bf16_rne(t)
        u = c["t16"].double() @ c["u"].double().t() + c["bias"].double()
        xn = c["x0"].double() * u + c["x"].double()
        dt = (du @ c["u"]).double()
        c["dt16"] = D.to_bf16_rne(dt)
        gp = c["g"].double() + c["dt16"].double() @ c["v"].double()
        exact += [t, u, xn, dt]
        if d == 429:   # the roundings are really exercised
            assert min(D.inexact_fraction(t), D.inexact_fraction(dt)) >= 0.05
        c["u16"], c["xn"] = D.to_bf16_rne(u), xn.float()
        c["xn16"] = D.to_bf16_rne(xn)
    assert all(float(v.abs().max()) < EXACT_LIMIT for v in exact + [gp])
    c["gp"] = gp.float()
    return c


@pytest.mark.parametrize("shape", LR_SHAPES, ids=str)
def test_low_rank_forward_bit_exact(shape):
    """The two launches the node's low-rank forward is made of."""
    c, e = int_case(*shape), _ext()
    t16 = e.linear_fwd(_dev(c["a"].to(BF16)), _dev(c["v"].to(BF16)),
                       torch.Tensor(), 0)
    out = e.cross_fwd(t16, _dev(c["u"].to(BF16)), _dev(c["bias"]),
                      _dev(c["x0"].float()), _dev(c["x"].float()), True)
    for n, v in zip(("xn", "xn16", "u16", "t16"), (*out, t16)):
        _assert_bits_equal(v, c[n], f"{shape} {n}")


def _check_backward(c, shape, run):
    """run(g, x0, u16, dx0) -> outputs by name; dx0 is updated in place."""
    dx0 = _dev(c["dx0"].float())
    out = run(_dev(c["g"].float()), _dev(c["x0"].float()),
              _dev(c["us"].to(BF16)), dx0)
    out["dx0n"] = dx0
    for n, v in out.items():
        _assert_bits_equal(v, c[n], f"{shape} {n}")


@pytest.mark.parametrize("shape", LR_SHAPES, ids=str)
def test_low_rank_backward_bit_exact(shape):
    c = int_case(*shape)
    ut, vt = (_dev(c[k].t().to(BF16)) for k in ("u", "v"))
    _check_backward(c, shape, lambda g, x0, u16, dx0: dict(zip(
        ("gp", "du16", "dt16"), _ext().cross_lr_bwd(g, x0, u16, ut, vt,
                                                    dx0))))


@pytest.mark.parametrize("shape", FULL_SHAPES, ids=str)
def test_full_matrix_backward_bit_exact(shape):
    c = int_case(*shape, 0)
    wt = _dev(c["w"].t().to(BF16))

    def run(g, x0, u16, dx0):
        du16 = _ext().cross_du(g, x0, u16, dx0)
        return {"du16": du16, "gp": _ext().cross_dx(du16, wt, g)}
    _check_backward(c, shape, run)


@pytest.mark.parametrize("r", [0, 129])
def test_rank_outside_the_limit_raises(r):
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa
    f = lambda *s: z(*s, dt=torch.float32)  # noqa: E731
    with pytest.raises(RuntimeError, match="rank"):
        _ext().cross_lr_bwd(f(4, 8), f(4, 8), z(4, 8), z(r, 8), z(8, r),
                            f(4, 8))


# ------------------------------------------------------------------ the node

def _plain64(x0, layers):
    x = x0
    for lay in layers:
        u = (x @ lay[0].t()) @ lay[1].t() if len(lay) == 3 else x @ lay[0].t()
        x = x0 * (u + lay[-1]) + x
    return x


def _stack64(x0, layers, gout, rounded):
    """The contract's forward and backward, written out in fp64 -> x_L and
    the gradients of x0 and of every parameter in layer order."""
    bf = (lambda v: v.float().to(BF16).double()) if rounded else (lambda v: v)
    x, saved = x0, []
    for lay in layers:
        a = bf(x)
        t = bf(a @ bf(lay[0]).t()) if len(lay) == 3 else a
        u = t @ bf(lay[-2]).t() + lay[-1]
        saved.append((a, t, bf(u)))
        x = x0 * u + x
    g, dx0, grads = gout, torch.zeros_like(x0), []
    for lay, (a, t, u16) in zip(reversed(layers), reversed(saved)):
        du = bf(g * x0)
        dx0 = dx0 + g * u16
        if len(lay) == 3:
            dt = bf(du @ bf(lay[1]))
            grads = [dt.t() @ a, du.t() @ t, du.sum(0)] + grads
            g = g + dt @ bf(lay[0])
        else:
            grads = [du.t() @ a, du.sum(0)] + grads
            g = g + du @ bf(lay[0])
    return x, [dx0 + g] + grads


def _e2e_case(d, r, b=33, n_layers=3):
    gen = _gen(d, r, b)
    layers = []
    for _ in range(n_layers):
        ws = ([randn_bf16(gen, d, d, scale=d ** -0.5)] if r == 0 else
              [randn_bf16(gen, r, d, scale=d ** -0.5),
               randn_bf16(gen, d, r, scale=r ** -0.5)])
        layers.append([w.double() for w in ws]
                      + [torch.randn(d, generator=gen).double() * 0.1])
    return (randn_bf16(gen, b, d).double(), layers,
            torch.randn(b, d, generator=gen).double())


def reference_noise(d, r):
    """(fp64 autograd gradients, storage noise per gradient) of a case."""
    x0, layers, gout = _e2e_case(d, r)
    leaves = [x0.clone().requires_grad_(True)] + [
        p.clone().requires_grad_(True) for lay in layers for p in lay]
    it = iter(leaves[1:])
    _plain64(leaves[0], [[next(it) for _ in lay] for lay in layers]
             ).backward(gout)
    ref = [p.grad for p in leaves]
    for got, want in zip(_stack64(x0, layers, gout, False)[1], ref):
        assert rel_l2(got, want) < 1e-12
    noisy = _stack64(x0, layers, gout, True)[1]
    return ref, [rel_l2(n, w) for n, w in zip(noisy, ref)]


@pytest.mark.parametrize("d,r", E2E_CASES)
def test_stack_gradients_against_fp64(d, r):
    x0, layers, gout = _e2e_case(d, r)
    ref, noise = reference_noise(d, r)
    net = _CrossNet(d, len(layers), v2=True, low_rank=r, fused_train=True)
    with torch.no_grad():
        for m, lay in zip(net.ws, layers):
            for lin, w in zip(m if r else [m], lay):
                lin.weight.copy_(w)
            (m[1] if r else m).bias.copy_(lay[-1])
    net = net.to(DEV)
    x = x0.float().to(DEV).requires_grad_(True)
    out = net(x)
    out.backward(gout.float().to(DEV))
    with torch.no_grad():
        _assert_bits_equal(out, net(x), "grad mode against no_grad output")
    got = [x.grad] + [p.grad for p in net.parameters()]
    assert len(got) == len(ref)
    for i, (gr, want, nz) in enumerate(zip(got, ref, noise)):
        ratio = rel_l2(gr.cpu(), want) / nz
        print(f"D={d} R={r} gradient {i}: error / storage noise {ratio:.2f}")
        assert E2E_NOISE_FLOOR <= ratio <= E2E_NOISE_FACTOR, (i, ratio)


@pytest.mark.parametrize("make", [
    lambda **kw: MLPerfDLRMDCN(**kw), lambda **kw: DCN(v2=True, **kw)],
    ids=["mlperf_dlrm_dcn", "dcnv2"])
def test_model_trains_one_eager_step(make):
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.optimizers import AdamAsyncOptimizer
    torch.manual_seed(0)
    m = make(device=DEV, bf16=True, fused_cross_train=True)
    assert list(m.state_dict()) == list(make(device=DEV).state_dict())
    ds = CriteoSyntheticDataset(batch_size=64, seed=3, device=DEV,
                                matrix_format=True)
    opt = AdamAsyncOptimizer(params=m.parameters(),
                             embedding_variables=m.embedding_variables())
    dense, ids, labels = ds.next_batch()
    loss = m.loss_fn(m(dense, ids), labels)
    opt.zero_grad()
    loss.backward()
    grads = [p.grad for p in m.cross.parameters()]
    opt.step()
    assert torch.isfinite(loss)
    assert all(g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
               for g in grads)
