"""MFMA linear kernels against exact references at ragged and zoo shapes.

Integer-valued bf16 operands make fwd / dX / dW exact in fp32 whatever the
accumulation order (tests/dense_reference.py; preconditions proven on the
CPU by tests/test_dense_reference.py), so the comparisons are bit-exact:
a dropped K tail, a duplicated chunk, a misplaced tile or a wrong rounding
changes an integer. Every operand is a contiguous view into a larger
buffer whose remainder is NaN, so a read past M, N or K that is used shows
up as NaN.

The tests that place an operand at an address the fresh-allocation cases
never produce (a workspace slice 4 bytes off 16-byte alignment, a bf16
weight at an odd element) are separate functions at the end of the file.
"""
import pytest
import torch

from tests import dense_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
SENTINEL = 12345.0


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _bf16_operand(values, offset=R.GUARD):
    """Exact values -> bf16 view inside a NaN-filled device buffer."""
    v16 = values.double().to(BF16)
    assert torch.equal(v16.double(), values.double())
    return R.carve(v16, DEV, offset=offset)[0]


def _assert_bits_equal(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{what}: {got.dtype}{tuple(got.shape)} vs " \
        f"{want.dtype}{tuple(want.shape)}"
    assert not torch.isnan(got.float()).any(), \
        f"{what}: NaN in the output — a guard band was read and used"
    idt = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.view(idt) != want.view(idt)
    if bad.any():
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; "
            f"first at {i}: got {got[i].item()}, want {want[i].item()}; "
            f"rows {idx[:, 0].unique().tolist()[:12]}, "
            f"cols {idx[:, -1].unique().tolist()[:12]}")


# ------------------------------------------------------------------ fwd

def _check_fwd(m, n, k, variant, act, with_bias, w_offset=R.GUARD):
    c = R.fwd_case(m, n, k)
    s = R.sigmoid_shift(c["ref"], c["bias"]) if act == 2 else 0
    x = _bf16_operand(c["x"])
    w = _bf16_operand(c["w"].double() * 2.0 ** -s, offset=w_offset)
    if with_bias:
        bias = R.carve(c["bias"], DEV)[0]
        pre = c["ref"].double() * 2.0 ** -s + c["bias"].double()
    else:
        bias = torch.empty(0, device=DEV)
        pre = c["ref"].double() * 2.0 ** -s
    out = _ext().linear_fwd(x, w, bias, act, variant)
    assert out.shape == (m, n) and out.dtype == BF16
    what = f"fwd {m}x{n}x{k} variant={variant} act={act} bias={with_bias}"
    if act == 2:
        assert float(pre.abs().max()) <= R.SIGMOID_LIMIT
        got = out.cpu().double()
        assert not torch.isnan(got).any(), what
        # one bf16 ulp of the fp64 sigmoid
        torch.testing.assert_close(got, torch.sigmoid(pre), rtol=2.0 ** -7,
                                   atol=0, msg=lambda s_: f"{what}: {s_}")
    else:
        _assert_bits_equal(out, R.to_bf16_rne(R.apply_act(pre, act)), what)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("variant", [-1, 1])
@pytest.mark.parametrize("m,n,k", R.FWD_SHAPES)
def test_linear_fwd_exact(m, n, k, variant, act, with_bias):
    _check_fwd(m, n, k, variant, act, with_bias)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("variant", [-1, 1])
def test_linear_fwd_nan_stays_in_its_row(variant, act):
    """One quiet NaN in x makes exactly that output row NaN; every other
    row is bit-identical to the clean run."""
    m, n, k = 80, 72, 45
    c = R.fwd_case(m, n, k)
    row, col = 37, 41
    x = _bf16_operand(c["x"])
    w = _bf16_operand(c["w"].double() * 2.0 ** -6)
    bias = R.carve(c["bias"], DEV)[0]
    clean = _ext().linear_fwd(x, w, bias, act, variant).cpu()
    assert not torch.isnan(clean.float()).any()
    x[row, col] = torch.nan
    dirty = _ext().linear_fwd(x, w, bias, act, variant).cpu()
    nan_rows = torch.isnan(dirty.float())
    assert nan_rows[row].all(), "the NaN did not reach every column"
    keep = torch.arange(m) != row
    assert not nan_rows[keep].any(), "the NaN leaked into another row"
    assert torch.equal(dirty[keep].view(torch.int16),
                       clean[keep].view(torch.int16))


# ------------------------------------------------------------------- dX

def _check_dx(m, n, k, w_offset=R.GUARD):
    c = R.dx_case(m, n, k)
    g = _bf16_operand(c["g"])
    w = _bf16_operand(c["w"], offset=w_offset)
    dx = _ext().linear_dx(g, w)
    assert dx.shape == (m, k) and dx.dtype == BF16
    _assert_bits_equal(dx, R.to_bf16_rne(c["ref"].double()),
                       f"dX {m}x{n}x{k}")


@pytest.mark.parametrize("m,n,k", R.DX_SHAPES)
def test_linear_dx_exact(m, n, k):
    _check_dx(m, n, k)


# ------------------------------------------------------------------- dW

def _check_dw_result(c, dw, db, want_bias, what):
    _assert_bits_equal(dw, c["dw"].float(), what + " dW")
    if want_bias:
        _assert_bits_equal(db, c["db"].float(), what + " dbias")
    else:
        assert db is None or db.numel() == 0


@pytest.mark.parametrize("want_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("variant", [-1, 0, 2])
@pytest.mark.parametrize("m,n,k", R.DW_SHAPES)
def test_linear_dw_exact(m, n, k, variant, want_bias):
    if (m, n, k) == R.DW_SHAPES[-1]:
        # this shape is here for the multi-chunk blocks of variant 2, the
        # last of which holds a single chunk; a change of the heuristic in
        # linear_dw_impl must not silently empty the case
        m_chunks, cpb = R.dw_cpb(m, n, k)
        assert cpb > 1 and m_chunks % cpb != 0
    c = R.dw_case(m, n, k)
    g = _bf16_operand(c["g"])
    x = _bf16_operand(c["x"])
    dw, db = _ext().linear_dw(g, x, want_bias, variant)
    assert dw.shape == (n, k) and dw.dtype == torch.float32
    _check_dw_result(c, dw, db, want_bias,
                     f"dW {m}x{n}x{k} variant={variant}")


def _check_dw_out(m, n, k, off, want_bias, variant=-1):
    """linear_dw_out into flat[off:off+sz]: the slice starts as NaN (the
    kernel must zero all of it, tail included), everything around it holds
    a sentinel (the kernel must not touch it)."""
    c = R.dw_case(m, n, k)
    g = _bf16_operand(c["g"])
    x = _bf16_operand(c["x"])
    sz = n * k + (n if want_bias else 0)
    flat = torch.full((off + sz + R.GUARD,), SENTINEL, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[off:off + sz] = torch.nan
    ws = flat[off:off + sz]
    dw, db = _ext().linear_dw_out(g, x, ws, want_bias, variant)
    assert dw.data_ptr() == ws.data_ptr() and dw.shape == (n, k)
    what = f"dW_out {m}x{n}x{k} off={off} variant={variant}"
    _check_dw_result(c, dw, db, want_bias, what)
    got = flat.cpu()
    want = torch.cat([c["dw"].reshape(-1), c["db"]]).float()[:sz]
    _assert_bits_equal(got[off:off + sz], want, what + " slice")
    assert R.outside_untouched(got, off, sz, SENTINEL), \
        what + ": wrote outside its slice"


@pytest.mark.parametrize("want_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("m,n,k", R.DW_OUT_SHAPES)
def test_linear_dw_out_slice_16_byte_aligned(m, n, k, off, want_bias):
    _check_dw_out(m, n, k, off, want_bias)


# ------------------------------------------------------------- act_bwd

@pytest.mark.parametrize("n", [5, 1003, 2048 * 8 + 3])
def test_act_bwd_tail(n):
    """n % 8 != 0: the vector body and the scalar tail meet exactly."""
    gen = torch.Generator().manual_seed(n)
    dy = torch.randint(-7, 8, (n,), generator=gen).to(BF16)
    out = (torch.randint(-4, 9, (n,), generator=gen).float() / 8).to(BF16)
    dy_d, out_d = R.carve(dy, DEV)[0], R.carve(out, DEV)[0]
    relu = _ext().act_bwd(dy_d, out_d, 1)
    want = torch.where(out.float() > 0, dy, torch.zeros_like(dy))
    _assert_bits_equal(relu, want, f"act_bwd relu n={n}")
    sig = _ext().act_bwd(dy_d, out_d, 2).cpu().double()
    o = out.double()
    # dy, out and 1 - out are exact; two fp32 products and one bf16
    # rounding stay within one bf16 ulp of the fp64 product
    torch.testing.assert_close(sig, dy.double() * o * (1 - o),
                               rtol=2.0 ** -7, atol=0)


# ---------------------------------------------------------- host checks

def _good(rows, cols):
    return torch.ones(rows, cols, device=DEV, dtype=BF16)


def _bad_variants(rows, cols):
    return {
        "transposed view": _good(cols, rows).t(),
        "column slice": _good(rows, cols + 8)[:, :cols],
        "fp32": torch.ones(rows, cols, device=DEV),
        "fp16": torch.ones(rows, cols, device=DEV, dtype=torch.float16),
    }


@pytest.mark.parametrize("kind", ["transposed view", "column slice", "fp32",
                                  "fp16"])
def test_bindings_reject_strided_and_non_bf16(kind):
    ext = _ext()
    m, n, k = 32, 16, 24
    bias = torch.zeros(n, device=DEV)
    bad = lambda r, c_: _bad_variants(r, c_)[kind]  # noqa: E731
    ws = torch.zeros(n * k + n, device=DEV)
    calls = {
        "fwd x": lambda: ext.linear_fwd(bad(m, k), _good(n, k), bias, 0),
        "fwd w": lambda: ext.linear_fwd(_good(m, k), bad(n, k), bias, 0),
        "dx g": lambda: ext.linear_dx(bad(m, n), _good(n, k)),
        "dx w": lambda: ext.linear_dx(_good(m, n), bad(n, k)),
        "dw g": lambda: ext.linear_dw(bad(m, n), _good(m, k), True),
        "dw x": lambda: ext.linear_dw(_good(m, n), bad(m, k), True),
        "dw_out g": lambda: ext.linear_dw_out(bad(m, n), _good(m, k), ws,
                                              True),
        "dw_out x": lambda: ext.linear_dw_out(_good(m, n), bad(m, k), ws,
                                              True),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: {kind} operand was accepted")
    assert bool((ws == 0).all()), "a rejected call still wrote"


def test_bindings_reject_mismatched_inner_dimensions():
    ext = _ext()
    m, n, k = 32, 16, 24
    bias = torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError):
        ext.linear_fwd(_good(m, k), _good(n, k + 8), bias, 0)
    with pytest.raises(RuntimeError):
        ext.linear_fwd(_good(m, k), _good(n, k), bias[:n - 1], 0)
    with pytest.raises(RuntimeError):
        ext.linear_dx(_good(m, n), _good(n + 16, k))
    with pytest.raises(RuntimeError):
        ext.linear_dw(_good(m, n), _good(m + 16, k), True)
    with pytest.raises(RuntimeError):
        ext.linear_dw_out(_good(m, n), _good(m + 16, k),
                          torch.zeros(n * k + n, device=DEV), True)
    with pytest.raises(RuntimeError):
        ext.linear_dw_out(_good(m, n), _good(m, k),
                          torch.zeros(n * k + n + 1, device=DEV), True)
    # the good call still goes through
    assert ext.linear_fwd(_good(m, k), _good(n, k), bias, 0).shape == (m, n)


@pytest.mark.parametrize("variant", [1, 3, -2])
def test_linear_dw_rejects_unknown_variant(variant):
    """Only -1, 0 and 2 name a kernel; anything else raises before the
    workspace is zero-filled or a kernel runs."""
    ext = _ext()
    m, n, k = 32, 16, 24
    g, x = _good(m, n), _good(m, k)
    ws = torch.full((n * k + n,), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="linear_dw: variant"):
        ext.linear_dw(g, x, True, variant)
    with pytest.raises(RuntimeError, match="linear_dw_out: variant"):
        ext.linear_dw_out(g, x, ws, True, variant)
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all()), "a rejected call still wrote"


def test_linear_dw_valid_variants_agree():
    """-1, 0 and 2 go through both bindings and give the same bits
    (integer-valued operands: fp32 accumulation is exact in any order)."""
    ext = _ext()
    m, n, k = 32, 16, 24
    c = R.dw_case(m, n, k)
    g, x = _bf16_operand(c["g"]), _bf16_operand(c["x"])
    for variant in (-1, 0, 2):
        ws = torch.full((n * k + n,), torch.nan, device=DEV)
        for dw, db in (ext.linear_dw(g, x, True, variant),
                       ext.linear_dw_out(g, x, ws, True, variant)):
            _check_dw_result(c, dw, db, True, f"dW variant={variant}")


@pytest.mark.parametrize("variant", [2, 5, -2])
def test_linear_fwd_rejects_unknown_variant(variant):
    ext = _ext()
    m, n, k = 32, 16, 24
    bias = torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError, match="linear_fwd: variant"):
        ext.linear_fwd(_good(m, k), _good(n, k), bias, 0, variant)
    assert ext.linear_fwd(_good(m, k), _good(n, k), bias, 0).shape == (m, n)


# ------------------------------------------ module level, realistic values

def _graph_node_names(fn):
    seen, names, todo = set(), [], [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo.extend(nf for nf, _ in f.next_functions)
    return names


def _assert_within(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    assert not torch.isnan(err).any(), what
    over = err > bound
    if over.any():
        i = tuple(over.nonzero()[0].tolist())
        raise AssertionError(
            f"{what}: {int(over.sum())} of {over.numel()} elements over the "
            f"bound; first at {i}: err {err[i].item():.3e} > "
            f"{bound[i].item():.3e} (ref {ref[i].item():.6g})")


def test_fused_tower_against_fp64():
    """fused_mlp([64, 1], 429) as the zoo builds its towers, M = 512, randn
    values on the bf16 grid. Per layer, against an fp64 reference of the
    same bf16 inputs and weights:
        |out - ref| <= 2**-8 |ref| + K 2**-23 (|x| @ |w|^T + |b|)
    — one bf16 rounding of the result plus fp32 accumulation over K terms;
    the same with GEMM-K = N for dX; the accumulation term alone (over M)
    for dW and db, which stay fp32. The second layer's reference takes the
    kernel's own bf16 activations (and the first layer's backward the
    kernel's own bf16 dX), so each bound covers one kernel."""
    from deeprec_amd.ops.fused_mlp import fused_mlp
    M, K, H = 512, 429, 64
    torch.manual_seed(11)
    mlp = fused_mlp([H, 1], K).to(DEV)
    x = torch.randn(M, K).to(BF16)
    go = torch.randn(M, 1).to(BF16)
    xd = x.to(DEV).requires_grad_(True)
    h1 = mlp[0](xd)
    h1.retain_grad()
    out = mlp[1](h1)
    assert out.shape == (M, 1) and out.dtype == BF16
    names = _graph_node_names(out.grad_fn)
    assert names.count("_FusedLinearBackward") == 2, names
    assert not [s for s in names if "mm" in s.lower()], names
    out.backward(go.to(DEV))
    torch.cuda.synchronize()

    u = 2.0 ** -23
    X, GO = x.double(), go.double()
    w1 = mlp[0].weight.detach().to(BF16).double().cpu()
    b1 = mlp[0].bias.detach().float().double().cpu()
    w2 = mlp[1].weight.detach().to(BF16).double().cpu()
    b2 = mlp[1].bias.detach().float().double().cpu()
    H1 = h1.detach().cpu().double()
    OUT = out.detach().cpu().double()

    # forward
    for name, got, a, w, b, red in (("fwd 429->64", h1, X, w1, b1, K),
                                    ("fwd 64->1", out, H1, w2, b2, H)):
        ref = torch.relu(a @ w.t() + b)
        bound = 2.0 ** -8 * ref.abs() + red * u * (a.abs() @ w.abs().t()
                                                   + b.abs())
        _assert_within(got, ref, bound, name)
    assert (H1 > 0).double().mean() > 0.2 and (OUT > 0).double().mean() > 0.2

    # backward of layer 2 (N = 1): relu mask from the kernel's own output
    g2 = GO * (OUT > 0)
    ref = g2 @ w2
    full, _ = R.linear_bounds(g2, w2, ref, 1)
    _assert_within(h1.grad, ref, full, "dX 64->1")
    ref = g2.t() @ H1
    _, acc = R.linear_bounds(g2.t(), H1, ref, M)
    _assert_within(mlp[1].weight.grad, ref, acc, "dW 64->1")
    _assert_within(mlp[1].bias.grad, g2.sum(0), M * u * g2.abs().sum(0),
                   "db 64->1")

    # backward of layer 1 (K = 429), from the kernel's own bf16 dX above
    g1 = h1.grad.detach().cpu().double() * (H1 > 0)
    ref = g1 @ w1
    full, _ = R.linear_bounds(g1, w1, ref, H)
    _assert_within(xd.grad, ref, full, "dX 429->64")
    ref = g1.t() @ X
    _, acc = R.linear_bounds(g1.t(), X, ref, M)
    _assert_within(mlp[0].weight.grad, ref, acc, "dW 429->64")
    _assert_within(mlp[0].bias.grad, g1.sum(0), M * u * g1.abs().sum(0),
                   "db 429->64")
    assert mlp[0].weight.grad.dtype == torch.float32
    assert float(g1.abs().max()) > 0


# ---------------------------------------------------------------------
# Operands at addresses that fresh allocations never have. FlatDenseAdam
# lays its [dW | db] gradient slices and bf16 weight shadows back to back,
# so after any N = 1 layer the next slice starts at an odd element: a
# 4-byte-aligned fp32 workspace and a 2-byte-aligned bf16 weight.
# ---------------------------------------------------------------------

@pytest.mark.parametrize("want_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("m,n,k", R.DW_OUT_SHAPES)
def test_linear_dw_out_slice_4_byte_aligned(m, n, k, off, want_bias):
    """The zero-fill stores its float4 body 16-byte aligned behind a
    scalar head of 3, 2 or 1 floats."""
    _check_dw_out(m, n, k, off, want_bias)


@pytest.mark.parametrize("variant", [-1, 1])
@pytest.mark.parametrize("m,n,k", [(16, 1, 64), (80, 72, 45),
                                   (80, 72, 429)])
def test_linear_fwd_weight_at_odd_element(m, n, k, variant):
    _check_fwd(m, n, k, variant, 1, True, w_offset=R.GUARD + 1)


@pytest.mark.parametrize("m,n,k", [(80, 127, 72), (130, 300, 45),
                                   (16, 1024, 429)])
def test_linear_dx_weight_at_odd_element(m, n, k):
    _check_dx(m, n, k, w_offset=R.GUARD + 1)


def test_flat_adam_slices_after_a_one_wide_layer():
    """Two [64, 1] towers under FlatDenseAdam: the second tower's gradient
    slices and weight shadows start at odd elements. Its gradients must
    equal, bit for bit, those the same layers produce into fresh
    workspaces (integer-valued data: fp32 accumulation is exact), and a
    backward must leave no NaN pre-fill behind in the flat buffer."""
    from deeprec_amd.ops.dense_adam import FlatDenseAdam
    from deeprec_amd.ops.fused_mlp import FusedLinear
    M, K = 64, 45
    gen = torch.Generator().manual_seed(5)

    def ints(*shape, lo=-3, hi=3):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()

    layers = []
    for n, k in ((8, K), (1, 8), (8, K), (1, 8)):
        lin = FusedLinear(k, n, relu=False)
        with torch.no_grad():
            lin.weight.copy_(ints(n, k))
            lin.bias.copy_(ints(n) * 0.5)
        layers.append(lin.to(DEV))
    x = ints(M, K).to(BF16).to(DEV)
    go = ints(M, 1).to(BF16).to(DEV)

    def run():
        outs = []
        for a, b in (layers[:2], layers[2:]):
            o = b(a(x))
            o.backward(go)
            outs.append(o.detach().cpu())
        return outs

    plain_out = run()
    plain = [(m.weight.grad.clone(), m.bias.grad.clone()) for m in layers]
    for m in layers:
        m.weight.grad = m.bias.grad = None
    adam = FlatDenseAdam(layers, lr=1e-3)
    offs = [off for off, _ in adam._slices]
    assert offs[1] % 4 == 0 and offs[2] % 2 == 1 and offs[3] % 2 == 1, offs
    adam.g.fill_(torch.nan)
    flat_out = run()
    for a, b in zip(plain_out, flat_out):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert not torch.isnan(adam.g).any()
    for m, (off, sz), (dw, db) in zip(layers, adam._slices, plain):
        n, k = m.out_features, m.in_features
        assert torch.equal(adam.g[off:off + n * k].view(n, k), dw)
        assert torch.equal(adam.g[off + n * k:off + sz], db)
