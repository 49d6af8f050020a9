"""Sequence kernels (attention, GRU / AUGRU, residual LayerNorm, L2 norm,
DIN features, masked softmax pool) against tests/seq_reference.py.

The extension entry points are called directly, with every operand a
contiguous view inside a NaN-filled buffer (a read past an operand that is
used shows up as NaN). Two kinds of comparison:

  * structure-exact cases, compared bit for bit: inputs chosen so that
    every intermediate is exact in fp32 (one live key, q = 0 over 2**k
    keys, integer operands, one-hot masks, alpha = 0 / 1);
  * random bf16-representable values against the fp64 reference of the
    same operation, every element inside the bound derived in
    seq_reference.py (proven sound on the CPU by test_seq_reference.py).

Two limits are not derived there, by necessity:
  * GRU forward: the error feeds back through the recurrence and tanhf /
    __expf differ from libm, so the kernel's h_out may deviate from fp64 by
    at most 64 * e32, e32 = max |fp32 CPU reference - fp64 reference| of the
    same case (32 for the fast exponential against fp32, 2 for another
    summation order). Observed max |kernel - fp64| / e32 on an MI355X:
        (B, T, H)      GRU    AUGRU
        (1, 1, 32)     2.25   0.97
        (5, 2, 1)      0.81   1.00
        (6, 7, 8)      1.00   0.88
        (7, 5, 21)     1.00   0.88
        (7, 5, 22)     0.90   0.98
        (9, 20, 32)    0.95   0.98
  * FusedGRU end to end: relative L2 error of each gradient at most 4x the
    storage noise of the case (seq_reference.gru_storage_noise): gates,
    dpre and h_prev are stored in bf16, and two GEMM roundings stack on
    top.
bf16 outputs of the GRU kernels may be one bf16 ulp off the rounded
reference on at most 1 % of the elements.
"""
import pytest
import torch

from tests import seq_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GRU_E32_FACTOR = 64.0
E2E_NOISE_FACTOR = 4.0

MHA_ALL = [(s, p) for s in R.MHA_SHAPES for p in R.MHA_PADS]
GRU_ALL = [(s, a) for s in R.GRU_SHAPES for a in (False, True)]


def _ids(cases):
    return ["-".join(str(x) for x in (c if isinstance(c, tuple) else (c,)))
            .replace("(", "").replace(")", "").replace(", ", "x")
            for c in cases]


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _dev(values):
    """values -> contiguous view inside a guard-banded device buffer: NaN
    around floating operands, 0xFF around uint8 masks."""
    fill = float("nan") if values.is_floating_point() else 255
    return R.carve(values.contiguous(), DEV, fill=fill)[0]


def _u8(mask):
    return _dev(mask.to(torch.uint8))


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


def _assert_values_equal(got, want, what):
    """Exact equality of the values (+0 and -0 are the same value)."""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double().reshape(got.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    bad = got != want
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
    assert n_ulp <= 1 and share <= R.FLIP_CAP, \
        f"{what}: up to {n_ulp:.2f} bf16 ulp off, {share:.4%} of the " \
        f"elements differ (allowed: 1 ulp, {R.FLIP_CAP:.0%})"


# -------------------------------------------------------------- attention

def _mha_run(c, pad, h, dout=None):
    ext = _ext()
    q, k, v = _dev(c["q"]), _dev(c["k"]), _dev(c["v"])
    pad_d = _u8(pad)
    out, stats = ext.mha_fwd(q, k, v, pad_d, h, c["scale"])
    got = {"out": out, "stats": stats}
    if dout is not None:
        dq, dk, dv = ext.mha_bwd(dout, q, k, v, pad_d, stats, h, c["scale"])
        got.update(dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return got


def _mha_check(shape, pad, what):
    b, t, d, h = shape
    c = R.mha_case(*shape)
    got = _mha_run(c, pad, h, _dev(c["dout"]))
    r = R.mha_ref(c["q"], c["k"], c["v"], pad, h, c["scale"], c["dout"])
    assert R.exp_precondition(r["arg"], r["live"])
    bound = R.mha_bounds(r, c["scale"])
    assert got["out"].dtype == BF16 and got["stats"].shape == (b, h, t, 2)
    for name in ("out", "dq", "dk", "dv"):
        R.assert_within(got[name], r[name], bound[name], f"{what} {name}")
    st = got["stats"].cpu()
    R.assert_within(st[..., 0], r["stats"][..., 0], bound["mx"],
                    f"{what} row max")
    R.assert_within(st[..., 1], r["stats"][..., 1], bound["sum"],
                    f"{what} row sum")
    dead = pad.all(1)
    for name in ("out", "dq", "dk", "dv"):
        _assert_zero(got[name][dead.to(DEV)], f"{what} {name} of a fully "
                     "padded sample")
    for name in ("dk", "dv"):
        _assert_zero(got[name][pad.to(DEV)], f"{what} {name} of padded keys")
    return c, got


@pytest.mark.parametrize("shape,pattern", MHA_ALL, ids=_ids(MHA_ALL))
def test_mha_against_fp64(shape, pattern):
    b, t, d, h = shape
    pad = R.mha_pad(b, t, pattern)
    c, got = _mha_check(shape, pad, f"mha {shape} {pattern}")
    if pattern == "last":
        # a single live key has probability exactly 1: out == v[live]
        want = c["v"][:, -1:, :].expand(b, t, d).contiguous()
        _assert_bits_equal(got["out"], want, f"mha {shape} one live key")


@pytest.mark.parametrize("dh", [4, 8, 16, 32])
def test_mha_uniform_attention_is_exact(dh):
    """q = 0 makes every score 0: over 8 live keys each probability is
    exactly 1/8. With small-integer k, v and dout, out and dv are exact
    dyadic numbers; where scale is a power of two (dh 4 and 16) so are dq
    and dk (= 0, q being 0). A sample with nothing live rides along."""
    b, t, h = 3, 16, 2
    d = dh * h
    gen = torch.Generator().manual_seed(dh)
    ri = lambda: torch.randint(-4, 5, (b, t, d), generator=gen)  # noqa: E731
    k, v, dout = ri(), ri(), ri()
    pad = torch.ones(b, t, dtype=torch.bool)
    for i in range(b - 1):
        live = torch.randperm(t, generator=gen)[:8]
        pad[i, live] = False
    scale = dh ** -0.5
    c = {"q": torch.zeros(b, t, d, dtype=BF16), "k": k.to(BF16),
         "v": v.to(BF16), "scale": scale}
    got = _mha_run(c, pad, h, _dev(dout.to(BF16)))
    r = R.mha_ref(c["q"], c["k"], c["v"], pad, h, scale, dout.to(BF16))
    assert float(r["p"][:b - 1].max()) == 0.125
    from tests.dense_reference import to_bf16_rne
    _assert_bits_equal(got["out"], to_bf16_rne(r["out"]), f"dh={dh} out")
    _assert_bits_equal(got["dv"], to_bf16_rne(r["dv"]), f"dh={dh} dv")
    st = got["stats"].cpu()
    assert bool((st[:b - 1, ..., 0] == 0).all())
    assert bool((st[:b - 1, ..., 1] == 8).all())
    assert bool((st[b - 1, ..., 0] == R.MHA_DEAD_MAX).all())
    assert bool((st[b - 1, ..., 1] == 0).all())
    _assert_zero(got["dk"], f"dh={dh} dk")        # q = 0
    if dh in (4, 16):
        assert scale in (0.5, 0.25)
        assert float(r["dq"].abs().max()) > 0
        _assert_bits_equal(got["dq"], to_bf16_rne(r["dq"]), f"dh={dh} dq")
    else:
        bound = R.mha_bounds(r, scale)
        R.assert_within(got["dq"], r["dq"], bound["dq"], f"dh={dh} dq")
    for name in ("out", "dq", "dk", "dv"):
        _assert_zero(got[name][b - 1], f"dh={dh} {name} of the dead sample")


def test_mha_bwd_takes_a_strided_dout():
    shape = (2, 17, 16, 4)
    b, t, d, h = shape
    c = R.mha_case(*shape)
    pad = R.mha_pad(b, t, "random")
    plain = _mha_run(c, pad, h, _dev(c["dout"]))
    wide = torch.full((b, t, 2 * d), float("nan"), dtype=BF16, device=DEV)
    wide[:, :, :d] = c["dout"].to(DEV)
    strided = wide[:, :, :d]
    assert not strided.is_contiguous()
    got = _mha_run(c, pad, h, strided)
    for name in ("dq", "dk", "dv"):
        _assert_bits_equal(got[name], plain[name], f"strided dout {name}")


def _mha_operands(b, t, d, h):
    mk = lambda: torch.zeros(b, t, d, dtype=BF16, device=DEV)  # noqa: E731
    pad = torch.zeros(b, t, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(b, h, t, 2, device=DEV)
    return mk(), mk(), mk(), mk(), pad, stats


def test_mha_bwd_rejects_an_lds_request_over_the_limit():
    """Backward at (1, 128, 256, 8) needs 8*T*D + 4*T*H = 266,240 bytes of
    LDS; the host check refuses it before anything is launched."""
    ext = _ext()
    b, t, d, h = 1, 128, 256, 8
    need = ext.mha_lds_bytes(t, d, h, True)
    assert need == 8 * t * d + 4 * t * h == 266240
    assert ext.mha_lds_bytes(t, d, h, False) == 4 * t * d
    limit = ext.mha_lds_limit()
    assert 0 < limit < need, limit
    dout, q, k, v, pad, stats = _mha_operands(b, t, d, h)
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        ext.mha_bwd(dout, q, k, v, pad, stats, h, 1.0)
    if ext.mha_lds_bytes(t, d, h, False) > limit:
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            ext.mha_fwd(q, k, v, pad, h, 1.0)
    # the limits forward always had hold for backward too
    dout, q, k, v, pad, stats = _mha_operands(1, 129, 32, 8)
    with pytest.raises(RuntimeError, match="sequence too long"):
        ext.mha_bwd(dout, q, k, v, pad, stats, 8, 1.0)
    dout, q, k, v, pad, stats = _mha_operands(1, 4, 64, 1)
    with pytest.raises(RuntimeError, match="head dim"):
        ext.mha_bwd(dout, q, k, v, pad, stats, 1, 1.0)
    dout, q, k, v, pad, stats = _mha_operands(1, 4, 12, 2)
    with pytest.raises(RuntimeError, match="head dim"):
        ext.mha_bwd(dout, q, k, v, pad, stats, 2, 1.0)
    torch.cuda.synchronize()


def test_mha_largest_admitted_shape_matches_the_reference():
    """D = 256, H = 8 (dh = 32) at the longest T whose backward request
    still fits the device's per-block LDS."""
    ext = _ext()
    d, h = 256, 8
    limit = ext.mha_lds_limit()
    t = min(1024 // h, limit // ext.mha_lds_bytes(1, d, h, True))
    assert t >= 8
    assert ext.mha_lds_bytes(t, d, h, True) <= limit
    assert t == 1024 // h or ext.mha_lds_bytes(t + 1, d, h, True) > limit
    shape = (2, t, d, h)
    print(f"per-block LDS limit {limit} B -> T = {t}: forward "
          f"{ext.mha_lds_bytes(t, d, h, False)} B, backward "
          f"{ext.mha_lds_bytes(t, d, h, True)} B")
    _mha_check(shape, R.mha_pad(2, t, "random"), f"mha {shape} at the limit")


def test_mha_bindings_reject_bad_operands():
    ext = _ext()
    b, t, d, h = 2, 8, 16, 2
    dout, q, k, v, pad, stats = _mha_operands(b, t, d, h)
    wide = torch.zeros(b, t, 2 * d, dtype=BF16, device=DEV)[:, :, :d]
    bad = {
        "fp32 q": lambda: ext.mha_fwd(q.float(), k, v, pad, h, 1.0),
        "fp32 k": lambda: ext.mha_fwd(q, k.float(), v, pad, h, 1.0),
        "fp16 v": lambda: ext.mha_fwd(q, k, v.half(), pad, h, 1.0),
        "strided q": lambda: ext.mha_fwd(wide, k, v, pad, h, 1.0),
        "strided k": lambda: ext.mha_fwd(q, wide, v, pad, h, 1.0),
        "short k": lambda: ext.mha_fwd(q, k[:, :t - 1].contiguous(), v, pad,
                                       h, 1.0),
        "bool pad": lambda: ext.mha_fwd(q, k, v, pad.bool(), h, 1.0),
        "short pad": lambda: ext.mha_fwd(q, k, v, pad[:, :t - 1].contiguous(),
                                         h, 1.0),
        "cpu v": lambda: ext.mha_fwd(q, k, v.cpu(), pad, h, 1.0),
        "bwd fp32 dout": lambda: ext.mha_bwd(dout.float(), q, k, v, pad,
                                             stats, h, 1.0),
        "bwd short dout": lambda: ext.mha_bwd(dout[:1], q, k, v, pad, stats,
                                              h, 1.0),
        "bwd strided v": lambda: ext.mha_bwd(dout, q, k, wide, pad, stats, h,
                                             1.0),
        "bwd fp32 q": lambda: ext.mha_bwd(dout, q.float(), k, v, pad, stats,
                                          h, 1.0),
        "bwd stats of another H": lambda: ext.mha_bwd(
            dout, q, k, v, pad, stats[:, :1].contiguous(), h, 1.0),
        "bwd bf16 stats": lambda: ext.mha_bwd(dout, q, k, v, pad,
                                              stats.to(BF16), h, 1.0),
        "bwd bool pad": lambda: ext.mha_bwd(dout, q, k, v, pad.bool(), stats,
                                            h, 1.0),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name} was accepted")
    out, st = ext.mha_fwd(q, k, v, pad, h, 1.0)       # the good call goes on
    assert out.shape == (b, t, d) and st.shape == (b, h, t, 2)
    assert ext.mha_bwd(dout, q, k, v, pad, st, h, 1.0)[0].shape == (b, t, d)


def test_fused_mha_function_is_the_kernels():
    """fused_mha's autograd wiring hands the kernels' results through
    unchanged."""
    from deeprec_amd.ops.fused_attention import fused_mha
    shape = (2, 20, 64, 8)
    b, t, d, h = shape
    c = R.mha_case(*shape)
    pad = R.mha_pad(b, t, "dead")
    direct = _mha_run(c, pad, h, _dev(c["dout"]))
    leaves = [c[n].to(DEV).requires_grad_(True) for n in "qkv"]
    out = fused_mha(*leaves, pad.to(DEV), h)
    out.backward(c["dout"].to(DEV))
    _assert_bits_equal(out, direct["out"], "fused_mha out")
    for name, leaf in zip(("dq", "dk", "dv"), leaves):
        _assert_bits_equal(leaf.grad, direct[name], f"fused_mha {name}")


# -------------------------------------------------------------------- GRU

def _gru_inputs(c):
    alpha = _dev(c["alpha"]) if c["alpha"] is not None else torch.Tensor()
    return _dev(c["X3"]), _dev(c["U"]), _dev(c["bh"]), alpha


@pytest.mark.parametrize("shape,augru", GRU_ALL, ids=_ids(GRU_ALL))
def test_gru_fwd_kernel(shape, augru):
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    x3, u, bh, alpha = _gru_inputs(c)
    h_out, gates = _ext().gru_fwd(x3, u, bh, alpha, b, t, h)
    torch.cuda.synchronize()
    assert h_out.shape == (b, t, h) and h_out.dtype == F32
    assert gates.shape == (b, t, 3 * h) and gates.dtype == BF16
    ref, gref = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    ref32, _ = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"], dtype=F32)
    e32 = float((ref32.double() - ref).abs().max())
    got = h_out.cpu().double()
    assert not torch.isnan(got).any()
    err = float((got - ref).abs().max())
    print(f"gru_fwd {shape} augru={augru}: max err {err:.3e}, e32 "
          f"{e32:.3e}, ratio {err / e32:.2f}")
    assert e32 > 0
    assert err <= GRU_E32_FACTOR * e32, \
        f"h_out off by {err:.3e} = {err / e32:.1f} x e32 ({e32:.3e})"
    _assert_ulp(gates, gref, f"gru_fwd {shape} augru={augru} gates")


@pytest.mark.parametrize("shape,augru", GRU_ALL, ids=_ids(GRU_ALL))
def test_gru_bwd_kernel(shape, augru):
    """gru_bwd on the reference's own h_out and gates: a pure function of
    exact inputs."""
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    h64, g64 = R.gru_fwd_ref(c["X3"], c["U"], c["bh"], c["alpha"])
    h32, g16 = h64.float(), g64.float().to(BF16)
    dpx, dph, da, da_b = R.gru_bwd_ref(c["dh_out"], h32, g16, c["U"],
                                       c["bh"], c["alpha"], with_bounds=True)
    alpha = _dev(c["alpha"]) if augru else torch.Tensor()
    got_x, got_h, got_a = _ext().gru_bwd(
        _dev(c["dh_out"]), _dev(h32), _dev(g16), _dev(c["U"]), _dev(c["bh"]),
        alpha, b, t, h)
    torch.cuda.synchronize()
    what = f"gru_bwd {shape} augru={augru}"
    _assert_ulp(got_x, dpx, what + " dpre_x")
    _assert_ulp(got_h, dph, what + " dpre_h")
    if augru:
        assert got_a.shape == (b, t) and got_a.dtype == F32
        R.assert_within(got_a, da, da_b, what + " dalpha")


@pytest.mark.parametrize("shape", R.GRU_SHAPES, ids=_ids(R.GRU_SHAPES))
def test_augru_alpha_one_is_the_plain_gru(shape):
    b, t, h = shape
    c = R.gru_case(b, t, h, False)
    x3, u, bh, _ = _gru_inputs(c)
    ext = _ext()
    h0, g0 = ext.gru_fwd(x3, u, bh, torch.Tensor(), b, t, h)
    h1, g1 = ext.gru_fwd(x3, u, bh, _dev(torch.ones(b, t)), b, t, h)
    _assert_bits_equal(h1, h0, f"alpha = 1 h_out {shape}")
    _assert_bits_equal(g1, g0, f"alpha = 1 gates {shape}")


@pytest.mark.parametrize("shape", [(7, 5, 21), (9, 20, 32)],
                         ids=["7x5x21", "9x20x32"])
def test_augru_alpha_zero_freezes_the_state(shape):
    """DIEN reads h_out[:, -1] as the final state and sends the gradient
    in there only: behind the last live step alpha is exactly 0, the state
    must not move, the frozen steps must get exactly zero dpre, and the
    gradient must arrive at the last live step unchanged — the live
    prefix's backward is, bit for bit, that of a run cut to its length."""
    b, t, h = shape
    c = R.gru_case(b, t, h, True)
    live = t - 2
    alpha = c["alpha"].clone()
    alpha[:, live:] = 0.0
    ext = _ext()
    x3, u, bh, _ = _gru_inputs(c)
    h_out, gates = ext.gru_fwd(x3, u, bh, _dev(alpha), b, t, h)
    for i in range(live, t):
        _assert_bits_equal(h_out[:, i], h_out[:, i - 1],
                           f"frozen state at step {i}")
    dh = torch.zeros(b, t, h)
    dh[:, -1] = c["dh_out"][:, -1]
    dpx, dph, da = ext.gru_bwd(_dev(dh), h_out, gates, u, bh, _dev(alpha), b,
                               t, h)
    _assert_zero(dpx[:, live:], "dpre_x of the frozen steps")
    _assert_zero(dph[:, live:], "dpre_h of the frozen steps")
    assert not torch.isnan(da).any()
    # the same gradient put straight onto the last live step of a cut run
    dh_cut = torch.zeros(b, live, h)
    dh_cut[:, -1] = c["dh_out"][:, -1]
    cx, chh, ca = ext.gru_bwd(
        _dev(dh_cut), _dev(h_out[:, :live].cpu()),
        _dev(gates[:, :live].cpu()), u, bh, _dev(alpha[:, :live]), b, live,
        h)
    assert float(cx.float().abs().max()) > 0
    _assert_bits_equal(dpx[:, :live].contiguous(), cx, "live dpre_x")
    _assert_bits_equal(dph[:, :live].contiguous(), chh, "live dpre_h")
    _assert_bits_equal(da[:, :live].contiguous(), ca, "live dalpha")


def test_gru_rejects_hidden_size_33():
    ext = _ext()
    b, t, h = 2, 3, 33
    x3 = torch.zeros(b, t, 3 * h, dtype=BF16, device=DEV)
    u = torch.zeros(3 * h, h, dtype=BF16, device=DEV)
    bh = torch.zeros(3 * h, device=DEV)
    with pytest.raises(RuntimeError, match="hidden size <= 32"):
        ext.gru_fwd(x3, u, bh, torch.Tensor(), b, t, h)
    with pytest.raises(RuntimeError, match="hidden size <= 32"):
        ext.gru_bwd(torch.zeros(b, t, h, device=DEV),
                    torch.zeros(b, t, h, device=DEV), x3, u, bh,
                    torch.Tensor(), b, t, h)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,augru", GRU_ALL, ids=_ids(GRU_ALL))
def test_fused_gru_end_to_end(shape, augru):
    """FusedGRU forward + backward against fp64 autograd of the forward
    with the bf16 roundings of x, W and X3 applied."""
    from deeprec_amd.ops.fused_gru import FusedGRU
    b, t, h = shape
    c = R.gru_case(b, t, h, augru)
    gru = FusedGRU(R.GRU_IN, h)
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
            ok = rel == 0.0                 # T = 1: dW_hh is exactly zero
        else:
            ok = rel <= E2E_NOISE_FACTOR * noise[k]
        if not ok:
            bad.append(k)
    report = f"FusedGRU {shape} augru={augru}\n  " + "\n  ".join(lines)
    print(report)
    assert not bad, f"over {E2E_NOISE_FACTOR} x storage noise: {bad}\n{report}"


# ------------------------------------------------------ residual LayerNorm

@pytest.mark.parametrize("m,n", R.RESLN_SHAPES, ids=_ids(R.RESLN_SHAPES))
def test_resln_against_fp64(m, n):
    ext = _ext()
    c = R.resln_case(m, n)
    gamma, beta = _dev(c["gamma"]), _dev(c["beta"])
    y, z, stats = ext.resln_fwd(_dev(c["x"]), _dev(c["a"]), gamma, beta,
                                R.RESLN_EPS)
    torch.cuda.synchronize()
    r = R.resln_fwd_ref(c["x"], c["a"], c["gamma"], c["beta"])
    fb = R.resln_fwd_bounds(r, c["gamma"], c["beta"])
    what = f"resln {m}x{n}"
    assert y.dtype == BF16 and z.dtype == BF16 and stats.shape == (m, 2)
    R.assert_within(y, r["y"], fb["y"], what + " y")
    R.assert_within(z, r["z"], fb["z"], what + " z")
    R.assert_within(stats, r["stats"], fb["stats"], what + " stats")
    # backward on the reference's own z and stats: exact inputs
    z16, st32 = r["z"].float().to(BF16), r["stats"].float()
    dz, dgamma, dbeta = ext.resln_bwd(_dev(c["dy"]), _dev(z16), _dev(st32),
                                      gamma)
    torch.cuda.synchronize()
    b = R.resln_bwd_ref(c["dy"], z16, st32, c["gamma"])
    bb = R.resln_bwd_bounds(b)
    R.assert_within(dz, b["dz"], bb["dz"], what + " dz")
    R.assert_within(dgamma, b["dgamma"], bb["dgamma"], what + " dgamma")
    R.assert_within(dbeta, b["dbeta"], bb["dbeta"], what + " dbeta")


def test_fused_residual_ln_module_is_the_kernels():
    """FusedResidualLN hands the kernels' results through: y unchanged,
    dz to BOTH residual inputs."""
    from deeprec_amd.ops.fused_attention import FusedResidualLN
    m, n = 257, 32
    c = R.resln_case(m, n)
    ext = _ext()
    ln = FusedResidualLN(n, eps=R.RESLN_EPS)
    with torch.no_grad():
        ln.weight.copy_(c["gamma"])
        ln.bias.copy_(c["beta"])
    ln.to(DEV)
    x = c["x"].to(DEV).requires_grad_(True)
    a = c["a"].to(DEV).requires_grad_(True)
    y = ln(x, a)
    y.backward(c["dy"].to(DEV))
    y0, z0, st0 = ext.resln_fwd(x.detach(), a.detach(), ln.weight.detach(),
                                ln.bias.detach(), R.RESLN_EPS)
    dz, dgamma, dbeta = ext.resln_bwd(c["dy"].to(DEV), z0, st0,
                                      ln.weight.detach())
    _assert_bits_equal(y, y0, "module y")
    _assert_bits_equal(x.grad, dz, "module dx")
    _assert_bits_equal(a.grad, dz, "module da")
    # dgamma / dbeta are atomic sums: equal up to the summation order
    b = R.resln_bwd_ref(c["dy"], z0.cpu(), st0.cpu(), c["gamma"])
    bb = R.resln_bwd_bounds(b)
    R.assert_within(ln.weight.grad, b["dgamma"], bb["dgamma"], "module dgamma")
    R.assert_within(ln.bias.grad, b["dbeta"], bb["dbeta"], "module dbeta")


# ---------------------------------------------------------------- l2norm

@pytest.mark.parametrize("m,n", R.L2NORM_SHAPES, ids=_ids(R.L2NORM_SHAPES))
def test_l2norm_against_fp64(m, n):
    ext = _ext()
    c = R.l2norm_case(m, n)
    y, inv = ext.l2norm_fwd(_dev(c["x"]), R.L2NORM_EPS)
    torch.cuda.synchronize()
    r = R.l2norm_fwd_ref(c["x"])
    fb = R.l2norm_fwd_bounds(r)
    what = f"l2norm {m}x{n}"
    R.assert_within(y, r["y"], fb["y"], what + " y")
    R.assert_within(inv, r["inv"], fb["inv"], what + " inv")
    if m >= 5:
        _assert_zero(y[3], what + " all-zero row")
    y16, inv32 = r["y"].float().to(BF16), r["inv"].float()
    dx = ext.l2norm_bwd(_dev(c["dy"]), _dev(y16), _dev(inv32))
    torch.cuda.synchronize()
    b = R.l2norm_bwd_ref(c["dy"], y16, inv32)
    R.assert_within(dx, b["dx"], R.l2norm_bwd_bounds(b)["dx"], what + " dx")


# -------------------------------------------------------------- din_feat

@pytest.mark.parametrize("b,t,d", R.DIN_SHAPES, ids=_ids(R.DIN_SHAPES))
def test_din_feat_exact(b, t, d):
    ext = _ext()
    c = R.din_case(b, t, d)
    seq, tgt = _dev(c["seq"].float()), _dev(c["tgt"].float())
    out = ext.din_feat_fwd(seq, tgt)
    assert out.shape == (b * t, 4 * d) and out.dtype == BF16
    _assert_bits_equal(out, c["out_f"].to(BF16), f"din fwd {b}x{t}x{d}")
    dseq, dtgt = ext.din_feat_bwd(_dev(c["g"].double().to(BF16)), seq, tgt)
    _assert_bits_equal(dseq, c["dseq"].float(), f"din dseq {b}x{t}x{d}")
    _assert_bits_equal(dtgt, c["dtgt"].float(), f"din dtgt {b}x{t}x{d}")


def test_empty_batch_is_no_launch_error():
    """With the launch status checked, an empty grid would raise: the
    bindings return empty results without launching."""
    ext = _ext()
    t, d, h = 5, 8, 2
    seq = torch.zeros(0, t, d, device=DEV)
    tgt = torch.zeros(0, d, device=DEV)
    out = ext.din_feat_fwd(seq, tgt)
    assert out.shape == (0, 4 * d)
    dseq, dtgt = ext.din_feat_bwd(out, seq, tgt)
    assert dseq.shape == (0, t, d) and dtgt.shape == (0, d)
    dout, q, k, v, pad, stats = _mha_operands(0, t, d, h)
    o, st = ext.mha_fwd(q, k, v, pad, h, 1.0)
    assert o.shape == (0, t, d) and st.shape == (0, h, t, 2)
    assert ext.mha_bwd(dout, q, k, v, pad, st, h, 1.0)[2].shape == (0, t, d)
    po, pw = ext.msm_pool_fwd(torch.zeros(0, t, device=DEV), seq,
                              torch.zeros(0, t, dtype=torch.uint8,
                                          device=DEV))
    assert po.shape == (0, d) and pw.shape == (0, t)
    torch.cuda.synchronize()


# -------------------------------------------------------------- msm_pool

@pytest.mark.parametrize("b,t,d", R.MSM_SHAPES, ids=_ids(R.MSM_SHAPES))
def test_msm_pool_against_fp64(b, t, d):
    ext = _ext()
    c = R.msm_case(b, t, d)
    seq, mask = _dev(c["seq"]), _u8(c["mask"])
    out, w = ext.msm_pool_fwd(_dev(c["scores"]), seq, mask)
    torch.cuda.synchronize()
    r = R.msm_fwd_ref(c["scores"], c["seq"], c["mask"])
    assert R.exp_precondition(r["arg"], c["mask"])
    fb = R.msm_fwd_bounds(r, c["seq"], c["mask"])
    what = f"msm_pool {b}x{t}x{d}"
    R.assert_within(w, r["w"], fb["w"], what + " w")
    R.assert_within(out, r["out"], fb["out"], what + " out")
    _assert_zero(w.cpu()[~c["mask"]], what + " w of masked positions")
    w32 = r["w"].float()
    dscores, dseq = ext.msm_pool_bwd(_dev(c["dout"]), seq, _dev(w32), mask)
    torch.cuda.synchronize()
    bw = R.msm_bwd_ref(c["dout"], c["seq"], w32, c["mask"])
    bb = R.msm_bwd_bounds(bw, c["mask"])
    R.assert_within(dscores, bw["dscores"], bb["dscores"], what + " dscores")
    R.assert_within(dseq, bw["dseq"], bb["dseq"], what + " dseq")


@pytest.mark.parametrize("b,t,d", R.MSM_SHAPES[1:],
                         ids=_ids(R.MSM_SHAPES[1:]))
def test_msm_pool_structure_exact(b, t, d):
    """Row 0: one valid position (w = 1 there: out == seq[t], dscores == 0,
    dseq == dout at t). Row 1: equal scores over 8 valid positions and
    integer seq / dout (an exact mean). Last row: nothing valid (zeros both
    ways)."""
    assert b >= 2 and t >= 8
    ext = _ext()
    gen = torch.Generator().manual_seed(b * 1000 + t + d)
    scores = torch.randn(b, t, generator=gen)
    seq = torch.randint(-8, 9, (b, t, d), generator=gen).float()
    dout = torch.randint(-8, 9, (b, d), generator=gen).float()
    mask = torch.zeros(b, t, dtype=torch.bool)
    hot = t - 1             # beyond the first 128 where T > 128
    mask[0, hot] = True
    if b > 2:
        valid = torch.randperm(t, generator=gen)[:8]
        mask[1, valid] = True
        scores[1] = 0.75
    seq_d, mask_d = _dev(seq), _u8(mask)
    out, w = ext.msm_pool_fwd(_dev(scores), seq_d, mask_d)
    dscores, dseq = ext.msm_pool_bwd(_dev(dout), seq_d, w, mask_d)
    torch.cuda.synchronize()
    onehot = torch.zeros(t)
    onehot[hot] = 1.0
    _assert_values_equal(w[0], onehot, "one-hot w")
    _assert_values_equal(out[0], seq[0, hot], "one-hot out")
    _assert_zero(dscores[0], "one-hot dscores")
    _assert_values_equal(dseq[0], onehot[:, None] * dout[0][None, :],
                         "one-hot dseq")
    if b > 2:
        wm = mask[1].double() / 8
        _assert_values_equal(w[1], wm, "uniform w")
        mean = (wm[:, None] * seq[1].double()).sum(0)
        _assert_values_equal(out[1], mean, "uniform out (exact mean)")
        _assert_values_equal(dseq[1], wm[:, None] * dout[1].double()[None, :],
                             "uniform dseq")
        sdot = seq[1].double() @ dout[1].double()
        want = wm * (sdot - (wm * sdot).sum())
        _assert_values_equal(dscores[1], want, "uniform dscores")
    for name, ten in (("w", w), ("out", out), ("dscores", dscores),
                      ("dseq", dseq)):
        _assert_zero(ten[b - 1], f"fully masked {name}")
