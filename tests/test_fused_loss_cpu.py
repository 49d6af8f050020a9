"""The fused BCE-with-logits reference formulas and bound arithmetic
(tests/loss_reference.py), checked without a GPU: the fp64 reference
against torch's own double-precision loss and autograd, the reduction
depth, and an fp32 emulation of the kernel's evaluation and summation
order against the bound the GPU test asserts."""
import pytest
import torch
import torch.nn.functional as F

from tests import loss_reference as R

SIZES = [1, 63, 64, 65, 1024, 1025, 8192]


@pytest.mark.parametrize("labels", ["hard", "soft"])
@pytest.mark.parametrize("b", SIZES)
def test_reference_matches_torch_double(b, labels):
    x, y = R.make_inputs(b, labels, seed=b)
    xd = x.double().requires_grad_()
    loss = F.binary_cross_entropy_with_logits(xd, y.double())
    assert abs(R.ref_loss(x, y) - float(loss)) <= 1e-13 * max(1, float(loss))
    (loss * 3.5).backward()
    ref = R.ref_grad(x, y, 3.5)
    # torch's double sigmoid(x) - y cancels near |x| = 88; ours does not
    assert torch.allclose(ref, xd.grad, rtol=1e-12, atol=2e-16 * 3.5 / b)


def test_fixed_points_are_in_the_inputs():
    x, _ = R.make_inputs(64, "hard", seed=0)
    assert x[:7].tolist() == [float(torch.tensor(v)) for v in R.FIXED_POINTS]
    x1, _ = R.make_inputs(1, "soft", seed=0)
    assert x1.tolist() == [0.0]


def test_reduction_depth():
    assert R.reduction_depth(1) == 1 + 10 + 1
    assert R.reduction_depth(1024) == 1 + 10 + 1
    assert R.reduction_depth(1025) == 2 + 10 + 1
    assert R.reduction_depth(8192) == 8 + 10 + 1


def test_reference_does_not_cancel_at_large_logits():
    x = torch.tensor([88.0, -88.0, 20.0])
    y = torch.tensor([1.0, 0.0, 1.0])
    g = R.ref_grad(x, y, 1.0) * 3
    assert g[0] < 0 and abs(float(g[0]) + 6.05e-39) < 1e-40
    assert g[1] > 0 and abs(float(g[1]) - 6.05e-39) < 1e-40
    assert abs(float(g[2]) + 2.0611536e-9) < 1e-15


@pytest.mark.parametrize("labels", ["hard", "soft"])
@pytest.mark.parametrize("b", SIZES)
def test_fp32_emulation_is_inside_the_forward_bound(b, labels):
    x, y = R.make_inputs(b, labels, seed=100 + b)
    got = R.emulate_fwd_fp32(x, y)
    err, bound = abs(got - R.ref_loss(x, y)), R.fwd_bound(x, y)
    print(f"B={b} {labels}: |err|={err:.3e} bound={bound:.3e}")
    assert err <= bound
    # the bound is a rounding bound, not a tolerance: a few ulp of the loss
    assert bound <= 64 * R.U * (float(x.abs().max()) + 1)


@pytest.mark.parametrize("labels", ["hard", "soft"])
def test_fp32_emulation_is_inside_the_backward_bound(labels):
    b, g = 8192, -2.75
    x, y = R.make_inputs(b, labels, seed=7)
    e = torch.exp(-x.abs())
    omy = 1 - y
    num = torch.where(x >= 0, torch.addcmul(omy, -y, e),
                      torch.addcmul(-y, e, omy))
    got = (num / (1 + e)) * (torch.tensor(g) / b)
    ref = R.ref_grad(x, y, g)
    assert bool(((got.double() - ref).abs() <= R.bwd_bound(ref, g, b)).all())
