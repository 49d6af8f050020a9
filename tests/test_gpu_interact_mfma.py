"""The MFMA pair-dot interaction kernels (ops/hip/interact_kernels.hip),
always called with variant=2.

Exact cases: integer inputs in [-2, 2] make every forward dot (|.| <= 64)
and every backward sum (|.| <= 126) exact in fp32 in any summation order
and exactly representable in bf16 (tests/interact_reference.py), so the
kernels must equal the int64 CPU reference bit for bit: zero tolerance.
Rounding cases: randn inputs on the bf16 grid against the fp64 reference
under the bounds derived in tests/interact_reference.py.

Every operand sits between two NaN-filled guards inside one larger
buffer, so a read outside a sample's rows shows in the result.
"""
import pytest
import torch

from tests import interact_reference as ir

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 16
GUARD = 1024          # elements; keeps the operand 16-byte aligned
MFMA, SCALAR, AUTO = 2, 1, 0


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _guarded(t):
    """t (CPU, any dtype holding bf16-exact values) -> a contiguous bf16
    device tensor in the middle of a NaN-filled buffer."""
    n = t.numel()
    buf = torch.full((GUARD + n + GUARD,), float("nan"),
                     dtype=torch.bfloat16, device=DEV)
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t.to(torch.bfloat16))
    return view


def _p_pad(f, extra=0):
    p = ir.n_pairs(f)
    return ((p + 15) & ~15) + extra


def _int_case(b, f, p_pad, head):
    """x [b, f, D], grad [b, head + p_pad], all integer; the grad's pad
    columns are nonzero."""
    p = ir.n_pairs(f)
    x = ir.int_tensor((b, f, D), 100 * f + b)
    grad = ir.int_tensor((b, head + p_pad), 100 * f + b + 1)
    grad[:, head + p:] = ir.nonzero_int_tensor((b, p_pad - p), 7)
    return x, grad


def _same(got, ref, what):
    """Bit-for-bit equality with the integer reference; prints where it
    fails first."""
    got, ref = got.cpu().double(), ref.double()
    bad = (got != ref) | got.isnan()
    if bad.any():
        idx = bad.nonzero()
        print(f"{what}: {idx.shape[0]} of {bad.numel()} differ, first at "
              f"{idx[:8].tolist()}: got {got[bad][:8].tolist()}, "
              f"want {ref[bad][:8].tolist()}")
    assert not bad.any(), what


def _check_exact_cat(b, fe, p_pad):
    ext = _ext()
    f = fe + 1
    p = ir.n_pairs(f)
    x, grad = _int_case(b, f, p_pad, D)
    bot, emb = x[:, 0].contiguous(), x[:, 1:].contiguous()
    bot_g, emb_g, grad_g = _guarded(bot), _guarded(emb), _guarded(grad)
    out = ext.interact_cat_fwd(bot_g, emb_g, p_pad, MFMA)
    assert out.shape == (b, D + p_pad) and out.dtype == torch.bfloat16
    ref = ir.ref_cat_fwd(bot, emb, p_pad)
    _same(out, ref, "cat fwd")
    assert (out[:, D + p:] == 0).all()
    dbot, demb = ext.interact_cat_bwd(grad_g, bot_g, emb_g, MFMA)
    rb, re = ir.ref_cat_bwd(grad, bot, emb)
    _same(dbot, rb, "dbot")
    _same(demb, re, "demb")
    # other pad columns in the grad: same result
    grad2 = grad.clone()
    grad2[:, D + p:] = -grad2[:, D + p:]
    dbot2, demb2 = ext.interact_cat_bwd(_guarded(grad2), bot_g, emb_g, MFMA)
    assert torch.equal(dbot2, dbot) and torch.equal(demb2, demb)


def _check_exact_plain(b, f, p_pad):
    ext = _ext()
    p = ir.n_pairs(f)
    x, grad = _int_case(b, f, p_pad, 0)
    x_g, grad_g = _guarded(x), _guarded(grad)
    out = ext.interact_fwd(x_g, p_pad, MFMA)
    assert out.shape == (b, p_pad) and out.dtype == torch.bfloat16
    _same(out[:, :p], ir.ref_fwd(x), "fwd")
    assert (out[:, p:] == 0).all()
    dx = ext.interact_bwd(grad_g, x_g, MFMA)
    _same(dx, ir.ref_bwd(grad, x), "dfeats")
    grad2 = grad.clone()
    grad2[:, p:] = -grad2[:, p:]
    assert torch.equal(ext.interact_bwd(_guarded(grad2), x_g, MFMA), dx)


@pytest.mark.parametrize("b", [1, 5, 67])
@pytest.mark.parametrize("fe", [1, 15, 16, 26, 31])
def test_exact_cat(b, fe):
    _check_exact_cat(b, fe, _p_pad(fe + 1))


@pytest.mark.parametrize("b", [1, 5, 67])
@pytest.mark.parametrize("f", [2, 17, 27, 32])
def test_exact_plain(b, f):
    _check_exact_plain(b, f, _p_pad(f))


def test_exact_whole_extra_pad_group():
    """p_pad = P + 16: a whole extra group of zero columns (P = 351 is not
    a multiple of 8, so this is P_pad 352 + 16 at the workload's F)."""
    _check_exact_cat(5, 26, _p_pad(27, 16))
    _check_exact_plain(5, 27, _p_pad(27, 16))
    # and where P itself is a multiple of 16: F = 32, P = 496
    _check_exact_cat(5, 31, ir.n_pairs(32) + 16)


@pytest.mark.parametrize("b,fe", [(67, 26), (5, 31)])
def test_rounding_cat(b, fe):
    ext = _ext()
    f = fe + 1
    p, p_pad = ir.n_pairs(f), _p_pad(f)
    gen = torch.Generator().manual_seed(11 * b + fe)
    x = torch.randn(b, f, D, generator=gen).to(torch.bfloat16).double()
    grad = torch.randn(b, D + p_pad, generator=gen).to(torch.bfloat16).double()
    bot, emb = x[:, 0].contiguous(), x[:, 1:].contiguous()
    bot_g, emb_g, grad_g = _guarded(bot), _guarded(emb), _guarded(grad)
    out = ext.interact_cat_fwd(bot_g, emb_g, p_pad, MFMA).cpu().double()
    assert torch.equal(out[:, :D], bot)
    assert (out[:, D + p:] == 0).all()
    err = (out[:, D:D + p] - ir.ref_fwd(x)).abs()
    bound = ir.fwd_bound(x)
    print(f"fwd cat B={b} Fe={fe}: worst err/bound "
          f"{(err / bound).max().item():.4f}")
    assert (err <= bound).all()
    dbot, demb = ext.interact_cat_bwd(grad_g, bot_g, emb_g, MFMA)
    dx = torch.cat([dbot.unsqueeze(1), demb], dim=1).cpu().double()
    rb, re = ir.ref_cat_bwd(grad, bot, emb)
    ref = torch.cat([rb.unsqueeze(1), re], dim=1)
    berr = (dx - ref).abs()
    bbound = ir.bwd_bound(grad[:, D:], x, grad[:, :D])
    print(f"bwd cat B={b} Fe={fe}: worst err/bound "
          f"{(berr / bbound).max().item():.4f}")
    assert (berr <= bbound).all()


@pytest.mark.parametrize("b,f", [(67, 27), (5, 32)])
def test_rounding_plain(b, f):
    ext = _ext()
    p, p_pad = ir.n_pairs(f), _p_pad(f)
    gen = torch.Generator().manual_seed(13 * b + f)
    x = torch.randn(b, f, D, generator=gen).to(torch.bfloat16).double()
    grad = torch.randn(b, p_pad, generator=gen).to(torch.bfloat16).double()
    x_g, grad_g = _guarded(x), _guarded(grad)
    out = ext.interact_fwd(x_g, p_pad, MFMA).cpu().double()
    err = (out[:, :p] - ir.ref_fwd(x)).abs()
    bound = ir.fwd_bound(x)
    print(f"fwd B={b} F={f}: worst err/bound {(err / bound).max().item():.4f}")
    assert (err <= bound).all() and (out[:, p:] == 0).all()
    dx = ext.interact_bwd(grad_g, x_g, MFMA).cpu().double()
    berr = (dx - ir.ref_bwd(grad, x)).abs()
    bbound = ir.bwd_bound(grad, x)
    print(f"bwd B={b} F={f}: worst err/bound "
          f"{(berr / bbound).max().item():.4f}")
    assert (berr <= bbound).all()


def _close_to_scalar(new, old, ref, bound):
    """Both variants compute the same sums in another order, so each is
    within `bound` of the fp64 reference, and (triangle inequality: two
    roundings of one value to bf16 can land on different neighbours) they
    are within 2 * bound of each other."""
    new, old = new.cpu().double(), old.cpu().double()
    assert ((new - ref).abs() <= bound).all()
    assert ((old - ref).abs() <= bound).all()
    assert ((new - old).abs() <= 2 * bound).all()


def test_autograd_cat_matches_scalar_variant():
    from deeprec_amd.ops.fused_mlp import dot_interaction_cat
    b, fe = 64, 26
    f, p_pad = fe + 1, _p_pad(fe + 1)
    p = ir.n_pairs(f)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(b, f, D, generator=gen).to(torch.bfloat16)
    grad = torch.randn(b, D + p_pad, generator=gen).to(torch.bfloat16)
    res = {}
    for variant in (MFMA, SCALAR):
        bot = x[:, 0].to(DEV).requires_grad_(True)
        emb = x[:, 1:].contiguous().to(DEV).requires_grad_(True)
        out = dot_interaction_cat(bot, emb, p_pad, variant)
        out.backward(grad.to(DEV))
        res[variant] = (out.detach(),
                        torch.cat([bot.grad.unsqueeze(1), emb.grad], dim=1))
    xd, gd = x.double(), grad.double()
    _close_to_scalar(res[MFMA][0][:, D:D + p], res[SCALAR][0][:, D:D + p],
                     ir.ref_fwd(xd), ir.fwd_bound(xd))
    assert torch.equal(res[MFMA][0][:, :D].cpu(), x[:, 0])
    rb, re = ir.ref_cat_bwd(gd, xd[:, 0], xd[:, 1:])
    _close_to_scalar(res[MFMA][1], res[SCALAR][1],
                     torch.cat([rb.unsqueeze(1), re], dim=1),
                     ir.bwd_bound(gd[:, D:], xd, gd[:, :D]))


def test_autograd_plain_matches_scalar_variant():
    from deeprec_amd.ops.fused_mlp import dot_interaction
    b, f = 64, 26
    p, p_pad = ir.n_pairs(f), _p_pad(f)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(b, f, D, generator=gen).to(torch.bfloat16)
    grad = torch.randn(b, p_pad, generator=gen).to(torch.bfloat16)
    res = {}
    for variant in (MFMA, SCALAR):
        feats = x.to(DEV).requires_grad_(True)
        out = dot_interaction(feats, p_pad, variant)
        out.backward(grad.to(DEV))
        res[variant] = (out.detach(), feats.grad)
    xd, gd = x.double(), grad.double()
    _close_to_scalar(res[MFMA][0][:, :p], res[SCALAR][0][:, :p],
                     ir.ref_fwd(xd), ir.fwd_bound(xd))
    _close_to_scalar(res[MFMA][1], res[SCALAR][1], ir.ref_bwd(gd, xd),
                     ir.bwd_bound(gd, xd))


@pytest.mark.parametrize("f,d", [(27, 8), (33, 16)])
def test_dispatch_ineligible_shapes(f, d):
    """variant=0 on a shape the MFMA kernels do not serve runs the scalar
    kernels (bit for bit); variant=2 raises."""
    ext = _ext()
    b, p_pad = 5, _p_pad(f)
    gen = torch.Generator().manual_seed(f)
    x = torch.randn(b, f, d, generator=gen).to(torch.bfloat16).to(DEV)
    grad = torch.randn(b, d + p_pad, generator=gen).to(torch.bfloat16).to(DEV)
    bot, emb = x[:, 0].contiguous(), x[:, 1:].contiguous()
    gp = grad[:, d:].contiguous()
    assert torch.equal(ext.interact_fwd(x, p_pad, AUTO),
                       ext.interact_fwd(x, p_pad, SCALAR))
    assert torch.equal(ext.interact_bwd(gp, x, AUTO),
                       ext.interact_bwd(gp, x, SCALAR))
    assert torch.equal(ext.interact_cat_fwd(bot, emb, p_pad, AUTO),
                       ext.interact_cat_fwd(bot, emb, p_pad, SCALAR))
    for a, s in zip(ext.interact_cat_bwd(grad, bot, emb, AUTO),
                    ext.interact_cat_bwd(grad, bot, emb, SCALAR)):
        assert torch.equal(a, s)
    with pytest.raises(RuntimeError, match="MFMA"):
        ext.interact_fwd(x, p_pad, MFMA)
    with pytest.raises(RuntimeError, match="MFMA"):
        ext.interact_bwd(gp, x, MFMA)
    with pytest.raises(RuntimeError, match="MFMA"):
        ext.interact_cat_fwd(bot, emb, p_pad, MFMA)
    with pytest.raises(RuntimeError, match="MFMA"):
        ext.interact_cat_bwd(grad, bot, emb, MFMA)
