"""Tile-MFMA GRU / AUGRU kernels (gru_tile_fwd / gru_tile_bwd, H <= 64)
against tests/seq_reference.py, mirroring the GRU section of
tests/test_gpu_seq_kernels.py on the new entry points.

Every operand is a contiguous view inside a NaN-filled buffer, which is
what the zero padding of the tiles is up against: a read past an operand,
a padded K column that is not a real zero or a tile row of a sample >= B
that takes part in anything shows up as NaN.

Limits, each met by the fp32 model of the kernels alone
(tests/test_gru_tile_reference.py):
  * forward: max |h_out - fp64 reference| <= 64 * e32, e32 = max |fp32 CPU
    reference - fp64 reference| of the case; gates by the ulp rule (one
    bf16 ulp on at most 1 % of the elements);
  * backward on the reference's own h_out and gates: dpre_x / dpre_h by the
    ulp rule, dalpha inside gru_tile_reference.tile_bwd_ref's bound;
  * bit for bit: alpha = 1 is the plain GRU, alpha = 0 freezes the state
    and zeroes dpre, a sample's results do not depend on its tile row or
    its neighbours;
  * FusedGRU end to end at H in {36, 48, 63, 64} and at 32 with
    impl="tile": relative L2 error of each gradient at most 4x the storage
    noise of the case.

Observed max |kernel - fp64| / e32 on an MI355X:
    (B, T, H)      GRU    AUGRU
    (1, 1, 33)     1.00   1.14
    (5, 2, 1)      6.86   1.00
    (16, 3, 16)    5.05   1.73
    (7, 5, 32)     5.02   4.08
    (17, 7, 36)    5.36   3.33
    (15, 5, 48)    5.56   2.48
    (65, 4, 63)    4.43   3.33
    (9, 20, 64)    4.70   4.13
(the fp32 model gives 1.00 to 6.71 on the same cases). In the same run the
bf16 outputs were at most one ulp off on at most 0.03 % of the elements
(gates, dpre_x, dpre_h), and every end-to-end gradient was within 1.22x its
storage noise. dalpha's worst error / bound per shape, in table order:
0.001, 0.086, 0.024, 0.005, 0.019, 0.004, 0.004, 0.002. The bound is loose
for this kernel: its 2**-18 terms are slack for exact three-term operands
(tests/gru_tile_reference.py).
"""
import pytest
import torch

from tests import gru_tile_reference as TR
from tests import seq_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GRU_E32_FACTOR = 64.0       # 32: __expf against libm, 2: summation order
E2E_NOISE_FACTOR = 4.0

FREEZE_SHAPES = [(17, 7, 36), (9, 20, 64)]
ROW_SHAPES = [(17, 7, 36), (65, 4, 63)]
E2E_ALL = [(s, a) for s in TR.E2E_SHAPES for a in (False, True)]


def _ids(cases):
    return ["-".join(str(x) for x in (c if isinstance(c, tuple) else (c,)))
            .replace("(", "").replace(")", "").replace(", ", "x")
            for c in cases]


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _dev(values):
    """values -> contiguous view inside a NaN guard-banded device buffer."""
    return R.carve(values.contiguous(), DEV, fill=float("nan"))[0]


def _assert_bits_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{what}: {got.dtype}{tuple(got.shape)} vs " \
        f"{want.dtype}{tuple(want.shape)}"
    assert not torch.isnan(got.float()).any(), f"{what}: NaN in the output"
    idt = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.contiguous().view(idt) != want.contiguous().view(idt)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; "
            f"first at {i}: got {got[i].item()}, want {want[i].item()}")


def _assert_zero(t, what):
    t = t.detach().cpu().float()
    assert not torch.isnan(t).any(), f"{what}: NaN"
    assert not bool(t.any()), f"{what}: {int((t != 0).sum())} nonzero"


def _assert_ulp(got, ref64, what):
    got = got.detach().cpu()
    assert got.dtype == BF16
    assert not torch.isnan(got.float()).any(), f"{what}: NaN in the output"
    n_ulp, share = R.ulp_flips(got.reshape(ref64.shape), ref64)
    print(f"{what}: up to {n_ulp:.2f} ulp, {share:.4%} differ")
    assert n_ulp <= 1 and share <= R.FLIP_CAP, \
        f"{what}: up to {n_ulp:.2f} bf16 ulp off, {share:.4%} of the " \
        f"elements differ (allowed: 1 ulp, {R.FLIP_CAP:.0%})"


def _gru_inputs(c):
    alpha = _dev(c["alpha"]) if c["alpha"] is not None else torch.Tensor()
    return _dev(c["X3"]), _dev(c["U"]), _dev(c["bh"]), alpha


@pytest.mark.parametrize("shape,augru", TR.TILE_ALL, ids=_ids(TR.TILE_ALL))
def test_gru_tile_fwd_kernel(shape, augru):
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    x3, u, bh, alpha = _gru_inputs(c)
    h_out, gates = _ext().gru_tile_fwd(x3, u, bh, alpha, b, t, h)
    torch.cuda.synchronize()
    assert h_out.shape == (b, t, h) and h_out.dtype == F32
    assert gates.shape == (b, t, 3 * h) and gates.dtype == BF16
    ref, gref = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    ref32, _ = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"], dtype=F32)
    e32 = float((ref32.double() - ref).abs().max())
    got = h_out.cpu().double()
    assert not torch.isnan(got).any()
    err = float((got - ref).abs().max())
    print(f"gru_tile_fwd {shape} augru={augru}: max err {err:.3e}, e32 "
          f"{e32:.3e}, ratio {err / e32:.2f}")
    assert e32 > 0
    assert err <= GRU_E32_FACTOR * e32, \
        f"h_out off by {err:.3e} = {err / e32:.1f} x e32 ({e32:.3e})"
    _assert_ulp(gates, gref, f"gru_tile_fwd {shape} augru={augru} gates")


@pytest.mark.parametrize("shape,augru", TR.TILE_ALL, ids=_ids(TR.TILE_ALL))
def test_gru_tile_bwd_kernel(shape, augru):
    """gru_tile_bwd on the reference's own h_out and gates: a pure
    function of exact inputs."""
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    h64, g64 = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    h32, g16 = h64.float(), g64.float().to(BF16)
    dpx, dph, da, da_b = TR.tile_bwd_ref(c["dh_out"], h32, g16, c["U"],
                                         c["bh"], c["alpha"])
    alpha = _dev(c["alpha"]) if augru else torch.Tensor()
    got_x, got_h, got_a = _ext().gru_tile_bwd(
        _dev(c["dh_out"]), _dev(h32), _dev(g16), _dev(c["U"]), _dev(c["bh"]),
        alpha, b, t, h)
    torch.cuda.synchronize()
    what = f"gru_tile_bwd {shape} augru={augru}"
    assert got_x.shape == (b, t, 3 * h) and got_h.shape == (b, t, 3 * h)
    _assert_ulp(got_x, dpx, what + " dpre_x")
    _assert_ulp(got_h, dph, what + " dpre_h")
    if augru:
        assert got_a.shape == (b, t) and got_a.dtype == F32
        worst = float(((got_a.cpu().double() - da).abs()
                       / da_b.clamp(min=1e-300)).max())
        print(f"{what} dalpha: worst err / bound {worst:.3f}")
        R.assert_within(got_a, da, da_b, what + " dalpha")
    else:
        assert got_a is None or got_a.numel() == 0


@pytest.mark.parametrize("shape", TR.TILE_SHAPES, ids=_ids(TR.TILE_SHAPES))
def test_tile_alpha_one_is_the_plain_gru(shape):
    b, t, h = shape
    c = R.gru_case(b, t, h, False)
    x3, u, bh, _ = _gru_inputs(c)
    ext = _ext()
    h0, g0 = ext.gru_tile_fwd(x3, u, bh, torch.Tensor(), b, t, h)
    h1, g1 = ext.gru_tile_fwd(x3, u, bh, _dev(torch.ones(b, t)), b, t, h)
    _assert_bits_equal(h1, h0, f"alpha = 1 h_out {shape}")
    _assert_bits_equal(g1, g0, f"alpha = 1 gates {shape}")


@pytest.mark.parametrize("shape", FREEZE_SHAPES, ids=_ids(FREEZE_SHAPES))
def test_tile_alpha_zero_freezes_the_state(shape):
    """Behind the last live step alpha is exactly 0: the state must not
    move, the frozen steps must get exactly zero dpre, and the live
    prefix's backward is, bit for bit, that of a run cut to its length."""
    b, t, h = shape
    c = R.gru_case(b, t, h, True)
    live = t - 2
    alpha = c["alpha"].clone()
    alpha[:, live:] = 0.0
    ext = _ext()
    x3, u, bh, _ = _gru_inputs(c)
    h_out, gates = ext.gru_tile_fwd(x3, u, bh, _dev(alpha), b, t, h)
    for i in range(live, t):
        _assert_bits_equal(h_out[:, i], h_out[:, i - 1],
                           f"frozen state at step {i}")
    dh = torch.zeros(b, t, h)
    dh[:, -1] = c["dh_out"][:, -1]
    dpx, dph, da = ext.gru_tile_bwd(_dev(dh), h_out, gates, u, bh,
                                    _dev(alpha), b, t, h)
    _assert_zero(dpx[:, live:], "dpre_x of the frozen steps")
    _assert_zero(dph[:, live:], "dpre_h of the frozen steps")
    assert not torch.isnan(da).any()
    # the same gradient put straight onto the last live step of a cut run
    dh_cut = torch.zeros(b, live, h)
    dh_cut[:, -1] = c["dh_out"][:, -1]
    cx, chh, ca = ext.gru_tile_bwd(
        _dev(dh_cut), _dev(h_out[:, :live].cpu()),
        _dev(gates[:, :live].cpu()), u, bh, _dev(alpha[:, :live]), b, live,
        h)
    assert float(cx.float().abs().max()) > 0
    _assert_bits_equal(dpx[:, :live].contiguous(), cx, "live dpre_x")
    _assert_bits_equal(dph[:, :live].contiguous(), chh, "live dpre_h")
    _assert_bits_equal(da[:, :live].contiguous(), ca, "live dalpha")


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=_ids(ROW_SHAPES))
def test_tile_rows_are_independent(shape):
    """A sample's h_out, gates, dpre_x, dpre_h and dalpha from the batched
    call equal, bit for bit, those of a B = 1 call on that sample alone:
    sample 0, the last row of the first tile and the last sample (row 0 of
    a later tile)."""
    b, t, h = shape
    c = R.gru_case(b, t, h, True)
    ext = _ext()
    x3, u, bh, alpha = _gru_inputs(c)
    h_out, gates = ext.gru_tile_fwd(x3, u, bh, alpha, b, t, h)
    dh = _dev(c["dh_out"])
    dpx, dph, da = ext.gru_tile_bwd(dh, h_out, gates, u, bh, alpha, b, t, h)
    assert b > 16
    for s in (0, 15, b - 1):
        one = slice(s, s + 1)
        x1, a1 = _dev(c["X3"][one]), _dev(c["alpha"][one])
        h1, g1 = ext.gru_tile_fwd(x1, u, bh, a1, 1, t, h)
        what = f"{shape} sample {s}"
        _assert_bits_equal(h1, h_out[one], what + " h_out")
        _assert_bits_equal(g1, gates[one], what + " gates")
        px1, ph1, da1 = ext.gru_tile_bwd(
            _dev(c["dh_out"][one]), _dev(h_out[one].cpu()),
            _dev(gates[one].cpu()), u, bh, a1, 1, t, h)
        _assert_bits_equal(px1, dpx[one], what + " dpre_x")
        _assert_bits_equal(ph1, dph[one], what + " dpre_h")
        _assert_bits_equal(da1, da[one], what + " dalpha")


def test_gru_tile_rejects_hidden_size_65():
    ext = _ext()
    b, t, h = 2, 3, 65
    x3 = torch.zeros(b, t, 3 * h, dtype=BF16, device=DEV)
    u = torch.zeros(3 * h, h, dtype=BF16, device=DEV)
    bh = torch.zeros(3 * h, device=DEV)
    with pytest.raises(RuntimeError, match="hidden size <= 64"):
        ext.gru_tile_fwd(x3, u, bh, torch.Tensor(), b, t, h)
    with pytest.raises(RuntimeError, match="hidden size <= 64"):
        ext.gru_tile_bwd(torch.zeros(b, t, h, device=DEV),
                         torch.zeros(b, t, h, device=DEV), x3, u, bh,
                         torch.Tensor(), b, t, h)
    torch.cuda.synchronize()


def _end_to_end(shape, augru, **kw):
    from deeprec_amd.ops.fused_gru import FusedGRU
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    gru = FusedGRU(R.GRU_IN, h, **kw)
    assert gru.tile
    with torch.no_grad():
        gru.weight_ih_l0.copy_(c["w_ih"].float())
        gru.weight_hh_l0.copy_(c["U"].float())
        gru.bias_ih_l0.copy_(c["b_ih"])
        gru.bias_hh_l0.copy_(c["bh"])
    gru.to(DEV)
    x = c["x"].float().to(DEV).requires_grad_(True)
    alpha = c["alpha"].to(DEV).requires_grad_(True) if augru else None
    h_out = gru(x, alpha)
    h_out.backward(c["dh_out"].to(DEV))
    torch.cuda.synchronize()
    h_ref, ref = R.gru_autograd(c)
    got = {"x": x.grad, "w_ih": gru.weight_ih_l0.grad,
           "b_ih": gru.bias_ih_l0.grad, "w_hh": gru.weight_hh_l0.grad,
           "b_hh": gru.bias_hh_l0.grad}
    if augru:
        got["alpha"] = alpha.grad
    noise = R.gru_storage_noise(b, t, h, augru)
    assert set(got) == set(ref) == set(noise)
    lines, bad = [], []
    for k in sorted(got):
        g = got[k].detach().cpu()
        assert g.shape == ref[k].shape and not torch.isnan(g).any(), k
        rel = R.rel_l2(g, ref[k])
        lines.append(f"{k}: rel L2 {rel:.3e}, noise {noise[k]:.3e}, "
                     f"ratio {rel / noise[k] if noise[k] else 0.0:.2f}")
        if float(ref[k].norm()) == 0.0:
            ok = rel == 0.0
        else:
            ok = rel <= E2E_NOISE_FACTOR * noise[k]
        if not ok:
            bad.append(k)
    report = f"FusedGRU {shape} augru={augru} {kw}\n  " + "\n  ".join(lines)
    print(report)
    assert not bad, f"over {E2E_NOISE_FACTOR} x storage noise: {bad}\n{report}"


@pytest.mark.parametrize("shape,augru", E2E_ALL, ids=_ids(E2E_ALL))
def test_fused_gru_wide_end_to_end(shape, augru):
    """FusedGRU forward + backward through the tile kernels against fp64
    autograd of the forward with the bf16 roundings of x, W and X3."""
    _end_to_end(shape, augru)


@pytest.mark.parametrize("augru", [False, True], ids=["gru", "augru"])
def test_fused_gru_tile_impl_at_32_end_to_end(augru):
    _end_to_end((7, 5, 32), augru, impl="tile")


def test_reference_dien_trains_on_gpu():
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.models.sequence import DIEN
    from deeprec_amd.optimizers import AdagradOptimizer
    torch.manual_seed(0)
    m = DIEN(item_dim=36, gru_hidden=36, device=torch.device(DEV))
    assert m.gru.tile and m.augru.tile
    ds = CriteoSyntheticDataset(batch_size=64, device=torch.device(DEV),
                                seed=4)
    opt = AdagradOptimizer(params=m.parameters(),
                           embedding_variables=m.embedding_variables(),
                           learning_rate=0.01)
    for i in range(3):
        dense, ids, seq, target, labels = ds.next_seq_batch(seq_len=20)
        out = m(dense, ids[:, :m.num_sparse], seq, target)
        loss = m.loss_fn(out, labels)
        opt.zero_grad()
        loss.backward()
        for mod in (m.gru, m.augru):
            for name, p in mod.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all()
                assert float(p.grad.abs().max()) > 0, (i, name)
        opt.step()
        assert torch.isfinite(loss), i
