"""tests/interact_reference.py against torch's fp64 autograd on the CPU."""
import pytest
import torch

from tests import interact_reference as ir


def _autograd(x, g):
    x = x.clone().requires_grad_(True)
    f = x.shape[1]
    z = torch.bmm(x, x.transpose(1, 2))
    iu = torch.triu_indices(f, f, offset=1)
    out = z[:, iu[0], iu[1]]
    out.backward(g[:, :out.shape[1]])
    return out.detach(), x.grad


@pytest.mark.parametrize("b,f,d", [(3, 2, 16), (5, 17, 16), (4, 27, 16),
                                   (2, 32, 16), (3, 33, 8)])
def test_reference_matches_autograd(b, f, d):
    gen = torch.Generator().manual_seed(f)
    x = torch.randn(b, f, d, generator=gen, dtype=torch.float64)
    g = torch.randn(b, ir.n_pairs(f) + 5, generator=gen, dtype=torch.float64)
    out, dx = _autograd(x, g)
    torch.testing.assert_close(ir.ref_fwd(x), out, rtol=0, atol=1e-12)
    torch.testing.assert_close(ir.ref_bwd(g, x), dx, rtol=0, atol=1e-12)


def test_pair_order_is_the_closed_form():
    f = 27
    i, j = ir.pair_rows_cols(f)
    p = i * f - i * (i + 1) // 2 + (j - i - 1)
    assert torch.equal(p, torch.arange(ir.n_pairs(f)))


@pytest.mark.parametrize("fe", [1, 15, 26, 31])
def test_integer_reference_is_exact_and_small(fe):
    b, d = 7, 16
    p = ir.n_pairs(fe + 1)
    p_pad = (p + 15) & ~15
    bot = ir.int_tensor((b, d), 1)
    emb = ir.int_tensor((b, fe, d), 2)
    grad = ir.int_tensor((b, d + p_pad), 3)
    grad[:, d + p:] = ir.nonzero_int_tensor((b, p_pad - p), 4)
    out = ir.ref_cat_fwd(bot, emb, p_pad)
    dbot, demb = ir.ref_cat_bwd(grad, bot, emb)
    assert out.abs().max() <= 64 and (out[:, d + p:] == 0).all()
    assert max(dbot.abs().max(), demb.abs().max()) <= 126
    # the same through fp64 autograd, exactly
    bd = bot.double().requires_grad_(True)
    ed = emb.double().requires_grad_(True)
    x = torch.cat([bd.unsqueeze(1), ed], dim=1)
    z = torch.bmm(x, x.transpose(1, 2))
    iu = torch.triu_indices(fe + 1, fe + 1, offset=1)
    o = torch.cat([bd, z[:, iu[0], iu[1]]], dim=1)
    o.backward(grad[:, :d + p].double())
    assert torch.equal(o.detach(), out[:, :d + p].double())
    assert torch.equal(bd.grad, dbot.double())
    assert torch.equal(ed.grad, demb.double())
    # every value survives bf16
    for t in (out, dbot, demb):
        assert torch.equal(t.to(torch.bfloat16).to(torch.int64), t)
    # pad columns of the grad are not read
    grad2 = grad.clone()
    grad2[:, d + p:] = 0
    dbot2, demb2 = ir.ref_cat_bwd(grad2, bot, emb)
    assert torch.equal(dbot2, dbot) and torch.equal(demb2, demb)


def test_bounds_hold_for_fp32_sums_rounded_to_bf16():
    """An fp32 evaluation rounded once to bf16 (what the kernels do, in
    torch's summation order) lies within the bounds; the bounds are not
    vacuous (within 2x of one bf16 rounding for these sizes)."""
    b, f, d = 16, 27, 16
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(b, f, d, generator=gen).to(torch.bfloat16)
    g = torch.randn(b, ir.n_pairs(f), generator=gen).to(torch.bfloat16)
    direct = torch.randn(b, d, generator=gen).to(torch.bfloat16)
    out = ir.ref_fwd(x.float()).to(torch.bfloat16).double()
    ref = ir.ref_fwd(x.double())
    bound = ir.fwd_bound(x.double())
    assert ((out - ref).abs() <= bound).all()
    assert (bound <= 2 * ir.UBF * ref.abs() + 1e-4).all()
    dx32 = ir.ref_bwd(g.float(), x.float())
    dx32[:, 0] += direct.float()
    dx = dx32.to(torch.bfloat16).double()
    dref = ir.ref_bwd(g.double(), x.double())
    dref[:, 0] += direct.double()
    dbound = ir.bwd_bound(g, x, direct)
    assert ((dx - dref).abs() <= dbound).all()
    assert (dbound >= ir.UBF * dref.abs()).all()
