"""The DCNv2 cross forward kernel (ops/hip/cross_kernels.hip: cross_fwd)
and the fused inference forward of _CrossNet against the numerical contract
of docs/KERNELS.md.

Kernel, bit for bit: integer operands (a, W, x, x0 in [-4, 4], bias multiples
of 0.5) keep every value below 2**23, exact in fp32 in any summation order,
so an int64 reference has to match x_next, bf(x_next) and bf(u) exactly.
Every operand is a view inside a NaN-filled buffer.

Stack: relative L2 error of the fused no-grad output against the unrounded
fp64 forward, at most E2E_NOISE_FACTOR times the case's storage noise (the
fp64 forward with the contract's bf16 rounding of a_l against the one
without). x0 and the weights of these cases are bf16-representable. That
_CrossNet really took the kernel is asserted three ways: its output equals a
direct cross_net call bit for bit, differs from the fused=False output, and
its error is at least E2E_NOISE_FLOOR times the storage noise. The kernel
makes exactly the modelled roundings plus fp32 accumulation, whose relative
error (D * 2**-23 < 6e-5) is below 5 % of the noise (> 1.6e-3), so its ratio
cannot fall under 0.95; the fp32 layer-by-layer path sits near 0.

Observed on an MI355X: error / storage noise 1.00 at D = 45 and D = 429.
"""
import functools

import pytest
import torch

from deeprec_amd.models.zoo import _CrossNet
from deeprec_amd.ops.fused_cross import cross_net
from tests import dense_reference as D
from tests.seq_reference import randn_bf16, rel_l2, _gen

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E2E_NOISE_FACTOR = 4.0
E2E_NOISE_FLOOR = 0.5
EXACT_LIMIT = 2 ** 23       # half-integers below this are exact in fp32

FULL_SHAPES = [(1, 1, 1), (17, 72, 45), (80, 429, 429), (33, 100, 130)]
E2E_DIMS = [45, 429]


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _dev(values, offset=D.GUARD):
    return D.carve(values.contiguous(), DEV, offset=offset)[0]


def _assert_bits_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert not torch.isnan(got.float()).any(), f"{what}: NaN in the output"
    idt = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.contiguous().view(idt) != want.contiguous().view(idt)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} differ"


@functools.lru_cache(maxsize=None)
def int_case(b, d, k):
    """Operands and the exact results of one forward layer."""
    seed = 7000003 * b + 7001 * d + 13 * k
    rng = (-4, 4)
    c = {"a": D.int_matrix(b, k, rng, seed),
         "x": D.int_matrix(b, d, rng, seed + 1),
         "x0": D.int_matrix(b, d, rng, seed + 2),
         "w": D.int_matrix(d, k, rng, seed + 3),
         "bias": D.half_bias(d, seed + 4)}
    u = (c["a"] @ c["w"].t()).double() + c["bias"].double()
    xn = c["x0"].double() * u + c["x"].double()
    assert max(float(u.abs().max()), float(xn.abs().max())) < EXACT_LIMIT
    if 429 in (d, k):   # the rounding is really exercised
        assert D.inexact_fraction(u) >= 0.05
    c["u16"], c["xn"] = D.to_bf16_rne(u), xn.float()
    c["xn16"] = D.to_bf16_rne(xn)
    return c


def _run_fwd(c, save, rows=slice(None)):
    """cross_fwd on the case's rows -> dict of its outputs."""
    out = _ext().cross_fwd(_dev(c["a"][rows].to(BF16)), _dev(c["w"].to(BF16)),
                           _dev(c["bias"]), _dev(c["x0"][rows].float()),
                           _dev(c["x"][rows].float()), save)
    return dict(zip(("xn", "xn16", "u16"), out))


@pytest.mark.parametrize("shape", FULL_SHAPES, ids=str)
def test_forward_kernel_bit_exact(shape):
    c = int_case(*shape)
    for n, v in _run_fwd(c, True).items():
        _assert_bits_equal(v, c[n], f"{shape} {n}")
    bare = _run_fwd(c, False)
    _assert_bits_equal(bare["xn"], c["xn"], f"{shape} xn, nothing saved")
    assert bare["u16"].numel() == 0


def test_rows_are_independent():
    shape = (80, 429, 429)
    c = int_case(*shape)
    full = _run_fwd(c, True)
    for r in (0, 15, shape[0] - 1):
        for n, v in _run_fwd(c, True, slice(r, r + 1)).items():
            _assert_bits_equal(v, full[n][r:r + 1], f"row {r} {n}")


# ----------------------------------------------------------------- the stack

def _forward64(x0, layers, rounded):
    bf = (lambda v: v.float().to(BF16).double()) if rounded else (lambda v: v)
    x = x0
    for w, b in layers:
        x = x0 * (bf(x) @ w.t() + b) + x
    return x


@pytest.mark.parametrize("d", E2E_DIMS)
def test_fused_inference_forward(d, b=33, n_layers=3):
    gen = _gen(d, b)
    lay = [(randn_bf16(gen, d, d, scale=d ** -0.5),
            torch.randn(d, generator=gen) * 0.1) for _ in range(n_layers)]
    x0 = randn_bf16(gen, b, d)
    l64 = [(w.double(), bb.double()) for w, bb in lay]
    ref = _forward64(x0.double(), l64, False)
    noise = rel_l2(_forward64(x0.double(), l64, True), ref)
    nets = {}
    for fused in (True, False):
        net = _CrossNet(d, n_layers, v2=True, fused=fused)
        with torch.no_grad():
            for m, (w, bb) in zip(net.ws, lay):
                m.weight.copy_(w)
                m.bias.copy_(bb)
        nets[fused] = net.to(DEV)
    x0_dev = x0.float().to(DEV)
    with torch.no_grad():
        out, plain = nets[True](x0_dev), nets[False](x0_dev)
        direct = cross_net(x0_dev, [(w.to(DEV), bb.to(DEV)) for w, bb in lay])
    _assert_bits_equal(out, direct, "_CrossNet against cross_net")
    assert not torch.equal(out, plain), "the fused flag changed nothing"
    ratio = rel_l2(out.cpu(), ref) / noise
    print(f"D={d}: error / storage noise {ratio:.2f}")
    assert E2E_NOISE_FLOOR <= ratio <= E2E_NOISE_FACTOR
    # with a gradient wanted the layer-by-layer fp32 path runs
    _assert_bits_equal(nets[True](x0_dev), plain, "grad mode output")


def test_cross_net_refuses_what_it_cannot_serve():
    x0 = torch.zeros(16, 8, device=DEV)
    w, b = torch.zeros(8, 8, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="forward only"):
        cross_net(x0, [(w.requires_grad_(True), b)])
    with pytest.raises(ValueError, match="device"), torch.no_grad():
        cross_net(x0, [(w.cpu(), b)])
