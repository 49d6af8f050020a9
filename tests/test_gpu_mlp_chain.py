"""The fused MLP backward against the unfused path it replaces.

FusedMLP runs a FusedLinear stack as one autograd node: each dX kernel
applies the activation gradient of the layer below in its epilogue, a
tower's adjacent flat-gradient slices are cleared by one fill, and dX of
the first layer is skipped when the input needs no gradient. None of this
may change a bit, so every comparison here is bit-exact unless it says
otherwise, and the reference is always the existing unfused path
(linear_dx followed by act_bwd; the layers called one by one), never the
code under test. Operands are views into NaN-filled buffers
(tests/dense_reference.py): a read past an operand that is used shows up
as NaN.

At M = 80 every dW/db element receives exactly one atomic add (one 128-row
chunk), so the weight gradients are deterministic and compared bit for
bit; at M = 272 (three chunks) they are compared to an fp64 reference
within the fp32 accumulation bound of dense_reference.linear_bounds.
"""
import functools

import pytest
import torch

from tests import dense_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
WIDTHS = (45, 136, 72, 1)
# a hidden layer of 136 in second place: its dX has GEMM-K >= 128, takes the
# LDS-staged kernel, and the chain keeps linear_dx + act_bwd for it
WIDE_SECOND = (45, 72, 136, 1)
RELU_STACK = ("relu", "relu", None)
SIGMOID_STACK = ("sigmoid", "sigmoid", "sigmoid")


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _bits(t):
    t = t.detach().cpu()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _assert_bits_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{what}: {got.dtype}{tuple(got.shape)} vs " \
        f"{want.dtype}{tuple(want.shape)}"
    assert not torch.isnan(got.float()).any(), \
        f"{what}: NaN in the output — a guard band was read and used"
    bad = _bits(got) != _bits(want)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; "
            f"first at {i}: got {got[i].item()}, want {want[i].item()}")


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


# ------------------------------------------------------ fused dX epilogue

def _prev_out(m, k):
    """bf16 [m,k], multiples of 1/8 in [-0.5, 1], with +0.0 and -0.0."""
    gen = torch.Generator().manual_seed(7 * m + k)
    prev = (torch.randint(-4, 9, (m, k), generator=gen).float() / 8).to(BF16)
    prev[0, 0] = 0.0
    prev[0, 1] = -0.0
    prev[m - 1, k - 1] = -0.0
    prev[m - 1, k - 2] = 0.0
    assert _bits(prev)[0, 1] == -32768 and _bits(prev)[0, 0] == 0
    return prev


@pytest.mark.parametrize("act", [1, 2], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("m,n,k", R.DX_SHAPES)
def test_dx_epilogue_equals_dx_then_act_bwd(m, n, k, act):
    ext = _ext()
    c = R.dx_case(m, n, k)
    g = R.carve(c["g"].double().to(BF16), DEV)[0]
    w = R.carve(c["w"].double().to(BF16), DEV)[0]
    prev = _prev_out(m, k)
    prev_d, prev_flat, off = R.carve(prev, DEV)
    want = ext.act_bwd(ext.linear_dx(g, w), prev_d, act)
    got = ext.linear_dx(g, w, prev_d, act)
    what = f"dX+act {m}x{n}x{k} act={act}"
    assert got.shape == (m, k) and got.dtype == BF16
    _assert_bits_equal(got, want, what)
    assert R.outside_untouched(prev_flat, off, prev.numel(), float("nan"))
    # keyword form, and prev_act = 0 leaves dX plain
    _assert_bits_equal(ext.linear_dx(g, w, prev_out=prev_d, prev_act=act),
                       want, what + " (keywords)")
    _assert_bits_equal(ext.linear_dx(g, w, prev_d, 0), ext.linear_dx(g, w),
                       what + " (prev_act=0)")
    if act == 1:
        # and against the exact integer reference, independent of act_bwd
        dx = R.to_bf16_rne(c["ref"].double())
        _assert_bits_equal(
            got, torch.where(prev.float() > 0, dx, torch.zeros_like(dx)),
            what + " vs int64")
        masked = prev.float() <= 0
        assert masked[0, 1] and bool((_bits(got)[masked] == 0).all())


def test_dx_epilogue_rejects_bad_prev_out():
    ext = _ext()
    m, n, k = 32, 16, 24
    g = torch.ones(m, n, device=DEV, dtype=BF16)
    w = torch.ones(n, k, device=DEV, dtype=BF16)
    bad = {
        "wrong rows": torch.ones(m + 16, k, device=DEV, dtype=BF16),
        "wrong cols": torch.ones(m, k + 8, device=DEV, dtype=BF16),
        "shape of g": torch.ones(m, n, device=DEV, dtype=BF16),
        "1-D": torch.ones(m * k, device=DEV, dtype=BF16),
        "transposed view": torch.ones(k, m, device=DEV, dtype=BF16).t(),
        "column slice": torch.ones(m, k + 8, device=DEV, dtype=BF16)[:, :k],
        "fp32": torch.ones(m, k, device=DEV),
        "cpu": torch.ones(m, k, dtype=BF16),
    }
    for name, prev in bad.items():
        for act in (0, 1, 2):
            with pytest.raises(RuntimeError):
                ext.linear_dx(g, w, prev, act)
                pytest.fail(f"{name}: accepted with act={act}")
    good = torch.ones(m, k, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError):
        ext.linear_dx(g, w, good, 3)
    with pytest.raises(RuntimeError):
        ext.linear_dx(g, w, None, 1)
    assert ext.linear_dx(g, w, good, 1).shape == (m, k)


# ------------------------------------------------- chain against per-layer

def _stack(acts, seed, widths=WIDTHS):
    from deeprec_amd.ops.fused_mlp import FusedLinear, FusedMLP
    torch.manual_seed(seed)
    layers, d = [], widths[0]
    for h, a in zip(widths[1:], acts):
        layers.append(FusedLinear(d, h, activation=a))
        d = h
    return FusedMLP(*layers).to(DEV)


@functools.lru_cache(maxsize=None)
def _data(m, seed=0):
    """Input and output gradient on the bf16 grid (CPU, never modified)."""
    gen = torch.Generator().manual_seed(100 + m + seed)
    x = torch.randn(m, WIDTHS[0], generator=gen).to(BF16)
    go = torch.randn(m, WIDTHS[-1], generator=gen).to(BF16)
    return x, go


def _per_layer(mlp, x):
    """The unfused reference: nn.Sequential.forward, one node per layer."""
    return torch.nn.Sequential.forward(mlp, x)


def _run(mlp, m, chain, needs_grad, seed=0):
    x, go = _data(m, seed)
    xd = R.carve(x, DEV)[0].requires_grad_(needs_grad)
    god = R.carve(go, DEV)[0]
    for p in mlp.parameters():
        p.grad = None
    out = mlp(xd) if chain else _per_layer(mlp, xd)
    names = _graph_node_names(out.grad_fn)
    if chain:
        assert names.count("_FusedMLPChainBackward") == 1, names
        assert names.count("_FusedLinearBackward") == 0, names
    else:
        assert names.count("_FusedLinearBackward") == len(mlp), names
    out.backward(god)
    torch.cuda.synchronize()
    return {"out": out.detach().cpu(),
            "dx": None if xd.grad is None else xd.grad.cpu(),
            "grads": [(l.weight.grad.cpu().clone(), l.bias.grad.cpu().clone())
                      for l in mlp]}


@functools.lru_cache(maxsize=None)
def _reference(acts, m, needs_grad, seed=0):
    """Per-layer results of the stack every test below rebuilds from the
    same seed; computed once per configuration."""
    return _run(_stack(acts, 21), m, False, needs_grad, seed)


def _check_against(ref, got, what):
    _assert_bits_equal(got["out"], ref["out"], what + " out")
    for i, ((dw, db), (rdw, rdb)) in enumerate(zip(got["grads"],
                                                   ref["grads"])):
        _assert_bits_equal(dw, rdw, f"{what} dW[{i}]")
        _assert_bits_equal(db, rdb, f"{what} db[{i}]")
        assert float(rdw.abs().max()) > 0


@pytest.mark.parametrize("needs_grad", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("acts", [RELU_STACK, SIGMOID_STACK],
                         ids=["relu", "sigmoid"])
def test_chain_equals_per_layer(acts, needs_grad):
    m = 80
    ref = _reference(acts, m, needs_grad)
    got = _run(_stack(acts, 21), m, True, needs_grad)
    _check_against(ref, got, f"chain {acts[0]} M={m}")
    if needs_grad:
        _assert_bits_equal(got["dx"], ref["dx"], "chain input grad")
        assert float(ref["dx"].float().abs().max()) > 0
    else:
        assert got["dx"] is None and ref["dx"] is None


@pytest.mark.parametrize("widths,n_act_bwd", [(WIDTHS, 0), (WIDE_SECOND, 1)],
                         ids=["narrow", "wide-second"])
def test_chain_fuses_act_grad_below_the_lds_threshold(widths, n_act_bwd,
                                                      monkeypatch):
    """Which form the chain picks per layer, counted at the extension
    boundary (the calls still run): dX of a layer narrower than 128 carries
    the activation gradient of the layer below in its epilogue; a wider
    one is followed by act_bwd. Either way the results are the per-layer
    ones."""
    ext = _ext()
    act_calls, dx_fused = [], []
    real_act, real_dx = ext.act_bwd, ext.linear_dx

    def act_bwd(dy, out, act):
        act_calls.append(tuple(dy.shape))
        return real_act(dy, out, act)

    def linear_dx(g, w, prev_out=None, prev_act=0):
        dx_fused.append((g.shape[1], prev_out is not None and prev_act != 0))
        return real_dx(g, w, prev_out, prev_act)

    m = 80
    mlp = _stack(RELU_STACK, 21, widths)
    ref = _run(mlp, m, False, True)
    monkeypatch.setattr(ext, "act_bwd", act_bwd)
    monkeypatch.setattr(ext, "linear_dx", linear_dx)
    got = _run(mlp, m, True, True)
    assert len(act_calls) == n_act_bwd, act_calls
    assert dx_fused == [(widths[3], True), (widths[2], widths[2] < 128),
                        (widths[1], False)], dx_fused
    _check_against(ref, got, f"chain {widths}")
    _assert_bits_equal(got["dx"], ref["dx"], "input grad")


@pytest.mark.parametrize("needs_grad", [True, False], ids=["dx", "nodx"])
def test_chain_fp32_input_casts_dx_back(needs_grad):
    """An fp32 input off the bf16 grid: the chain rounds it once on the way
    in, and hands back an fp32 input gradient (the bf16 dX cast back) only
    when one is wanted."""
    m = 80
    mlp = _stack(RELU_STACK, 21)
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(m, WIDTHS[0], generator=gen)
    assert not R.bf16_exact(x)
    god = R.carve(_data(m)[1], DEV)[0]
    res = []
    for chain in (False, True):
        for p in mlp.parameters():
            p.grad = None
        xd = R.carve(x, DEV)[0].requires_grad_(needs_grad)
        out = mlp(xd) if chain else _per_layer(mlp, xd)
        names = _graph_node_names(out.grad_fn)
        assert ("_FusedMLPChainBackward" in names) == chain, names
        out.backward(god)
        res.append((out.detach(), xd.grad, mlp[0].weight.grad.clone()))
    (ro, rdx, rdw), (go_, gdx, gdw) = res
    _assert_bits_equal(go_, ro, "fp32-input out")
    _assert_bits_equal(gdw, rdw, "fp32-input dW[0]")
    if needs_grad:
        assert gdx.dtype == torch.float32 and gdx.shape == x.shape
        _assert_bits_equal(gdx, rdx, "fp32 input grad")
        assert R.bf16_exact(gdx.cpu()) and float(gdx.abs().max()) > 0
    else:
        assert gdx is None and rdx is None


def test_chain_falls_back_per_layer():
    """Ragged row counts, hooked layers and module-global hooks take the
    per-layer path."""
    mlp = _stack(RELU_STACK, 21)
    x = torch.randn(80, WIDTHS[0], device=DEV).to(BF16)
    handle = mlp[1].register_forward_hook(lambda *a: None)
    names = _graph_node_names(mlp(x).grad_fn)
    assert names.count("_FusedLinearBackward") == 3, names
    handle.remove()
    names = _graph_node_names(mlp(x).grad_fn)
    assert names.count("_FusedMLPChainBackward") == 1, names
    fired = []
    handle = torch.nn.modules.module.register_module_forward_hook(
        lambda mod, a, o: fired.append(type(mod).__name__))
    try:
        names = _graph_node_names(mlp(x).grad_fn)
    finally:
        handle.remove()
    assert names.count("_FusedLinearBackward") == 3, names
    assert fired.count("FusedLinear") == 3, fired
    names = _graph_node_names(mlp(x).grad_fn)
    assert names.count("_FusedMLPChainBackward") == 1, names
    names = _graph_node_names(mlp(x[:72]).grad_fn)
    assert "_FusedMLPChainBackward" not in names, names
    # a 3-D input is flattened over its leading dimensions
    out = mlp(x.view(5, 16, WIDTHS[0]))
    assert out.shape == (5, 16, 1)
    _assert_bits_equal(out.reshape(80, 1), _per_layer(mlp, x), "3-D input")


# ---------------------------------------------------------------- flat mode

def _flat_pair(interleaved):
    """Chains A and B under one FlatDenseAdam; A is the reference stack."""
    from deeprec_amd.ops.dense_adam import FlatDenseAdam
    from deeprec_amd.ops.fused_mlp import _adjacent_span
    a, b = _stack(RELU_STACK, 21), _stack(RELU_STACK, 22)
    layers = ([l for pair in zip(a, b) for l in pair] if interleaved
              else list(a) + list(b))
    adam = FlatDenseAdam(layers, lr=1e-3)
    span = _adjacent_span([l.dw_ws for l in a])
    if interleaved:
        assert span is None
    else:
        assert span is not None and span.data_ptr() == a[0].dw_ws.data_ptr()
        assert span.numel() == sum(l.dw_ws.numel() for l in a)
        # any order
        assert _adjacent_span([l.dw_ws for l in reversed(a)]).numel() == \
            span.numel()
    return a, b, adam


def _slices_of(adam, chain):
    out = []
    for l in chain:
        off, sz = adam._slices[adam.layers.index(l)]
        n, k = l.out_features, l.in_features
        g = adam.g.detach().cpu()
        out.append((g[off:off + n * k].view(n, k), g[off + n * k:off + sz]))
    return out


def _b_all_nan(adam, b):
    return all(bool(torch.isnan(dw).all() and torch.isnan(db).all())
               for dw, db in _slices_of(adam, b))


@pytest.mark.parametrize("interleaved", [False, True],
                         ids=["adjacent", "interleaved"])
def test_flat_mode_one_chunk(interleaved):
    m = 80
    ref = _reference(RELU_STACK, m, False)
    a, b, adam = _flat_pair(interleaved)
    adam.g.fill_(torch.nan)
    got = _run(a, m, True, False)
    _assert_bits_equal(got["out"], ref["out"], "flat out")
    for i, ((dw, db), (rdw, rdb)) in enumerate(zip(_slices_of(adam, a),
                                                   ref["grads"])):
        _assert_bits_equal(dw, rdw, f"flat dW[{i}]")
        _assert_bits_equal(db, rdb, f"flat db[{i}]")
    for l in a:
        assert l.weight.grad.data_ptr() == l.dw_ws.data_ptr()
    assert _b_all_nan(adam, b), "chain A's backward wrote B's slices"


@pytest.mark.parametrize("interleaved", [False, True],
                         ids=["adjacent", "interleaved"])
def test_flat_mode_fill_launches(interleaved, monkeypatch):
    """Adjacent slices: ONE zero_f32 over the tower's union, then every
    linear_dw_out with zero=False. Interleaved slices: no zero_f32, every
    linear_dw_out zero-fills its own slice. The calls are counted at the
    extension boundary and still run, so the results are checked too."""
    ext = _ext()
    fills, dw_zero = [], []
    real_fill, real_dw_out = ext.zero_f32, ext.linear_dw_out

    def zero_f32(ws):
        fills.append((ws.data_ptr(), ws.numel()))
        return real_fill(ws)

    def linear_dw_out(g, x, ws, want_bias, variant=-1, zero=True):
        dw_zero.append(zero)
        return real_dw_out(g, x, ws, want_bias, variant, zero)

    monkeypatch.setattr(ext, "zero_f32", zero_f32)
    monkeypatch.setattr(ext, "linear_dw_out", linear_dw_out)
    m = 80
    ref = _reference(RELU_STACK, m, False)
    a, b, adam = _flat_pair(interleaved)
    adam.g.fill_(torch.nan)
    _run(a, m, True, False)
    if interleaved:
        assert fills == [] and dw_zero == [True] * len(a), (fills, dw_zero)
    else:
        lo = min(l.dw_ws.data_ptr() for l in a)
        assert fills == [(lo, sum(l.dw_ws.numel() for l in a))], fills
        assert dw_zero == [False] * len(a), dw_zero
    for i, ((dw, db), (rdw, rdb)) in enumerate(zip(_slices_of(adam, a),
                                                   ref["grads"])):
        _assert_bits_equal(dw, rdw, f"dW[{i}]")
        _assert_bits_equal(db, rdb, f"db[{i}]")
    # the per-layer path keeps one fill per layer inside linear_dw_out
    del fills[:], dw_zero[:]
    _run(a, m, False, False)
    assert fills == [] and dw_zero == [True] * len(a), (fills, dw_zero)


@functools.lru_cache(maxsize=None)
def _fp64_reference(m):
    """dW/db of every layer of the relu stack in fp64, from the per-layer
    path's own bf16 activations and bf16 dX (so each bound covers one dW
    kernel), with the accumulation bound of R.linear_bounds."""
    mlp = _stack(RELU_STACK, 21)
    x, go = _data(m)
    h, hs = x.to(DEV), []
    for layer in mlp:
        h = layer(h)
        h.retain_grad()
        hs.append(h)
    h.backward(go.to(DEV))
    torch.cuda.synchronize()
    out = []
    for i in range(len(mlp)):
        hi = hs[i].detach().cpu().double()
        g = hs[i].grad.cpu().double() if i + 1 < len(mlp) else go.double()
        if mlp[i].activation == "relu":
            g = g * (hi > 0)
        xin = x.double() if i == 0 else hs[i - 1].detach().cpu().double()
        dw = g.t() @ xin
        _, acc = R.linear_bounds(g.t(), xin, dw, m)
        out.append((dw, acc, g.sum(0), m * 2.0 ** -23 * g.abs().sum(0)))
    return out


@pytest.mark.parametrize("interleaved", [False, True],
                         ids=["adjacent", "interleaved"])
def test_flat_mode_three_chunks(interleaved):
    m = 272
    a, b, adam = _flat_pair(interleaved)
    adam.g.fill_(torch.nan)
    _run(a, m, True, False)
    for i, ((dw, db), (rdw, bdw, rdb, bdb)) in enumerate(
            zip(_slices_of(adam, a), _fp64_reference(m))):
        for name, got, want, bound in ((f"dW[{i}]", dw, rdw, bdw),
                                       (f"db[{i}]", db, rdb, bdb)):
            err = (got.double() - want).abs()
            assert not torch.isnan(err).any(), f"{name}: NaN left behind"
            assert bool((err <= bound).all()), \
                f"{name}: max err {float(err.max()):.3e}, " \
                f"{int((err > bound).sum())} over the bound"
        assert float(rdw.abs().max()) > 0
    assert _b_all_nan(adam, b), "chain A's backward wrote B's slices"


# ------------------------------------------------------------------- replay

def test_flat_chain_replays_in_a_captured_graph():
    m = 80
    a, b, adam = _flat_pair(False)
    refs = [_reference(RELU_STACK, m, False, seed) for seed in (1, 2, 3)]
    x0, go0 = _data(m)
    sx, sgo = x0.to(DEV), go0.to(DEV)
    # warm up off the capture stream, as torch.cuda.graph asks
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a(sx).backward(sgo)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    adam.zero_grad()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a(sx)
        out.backward(sgo)
    torch.cuda.synchronize()
    for seed, ref in zip((1, 2, 3), refs):
        x, go = _data(m, seed)
        sx.copy_(x)
        sgo.copy_(go)
        adam.g.fill_(torch.nan)   # the captured fill has to clear this
        graph.replay()
        torch.cuda.synchronize()
        _assert_bits_equal(out, ref["out"], f"replay {seed} out")
        for i, ((dw, db), (rdw, rdb)) in enumerate(zip(_slices_of(adam, a),
                                                       ref["grads"])):
            _assert_bits_equal(dw, rdw, f"replay {seed} dW[{i}]")
            _assert_bits_equal(db, rdb, f"replay {seed} db[{i}]")
        assert _b_all_nan(adam, b)
    assert not torch.equal(refs[0]["grads"][0][0], refs[1]["grads"][0][0])


# ------------------------------------------------------------ pad_cast_bf16

@pytest.mark.parametrize("m", [16, 100])
def test_pad_cast_bf16(m):
    k, kp = 13, 16
    gen = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=gen) * 3
    # ties between bf16 neighbours (round to even both ways), signed
    # zeros, the largest finite bf16 and a value that rounds up to inf
    x[0, :8] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, 0.0,
                             3.3895313892515355e38, 3.4e38, -1 - 2.0 ** -8,
                             2.0 ** -100 * (1 + 2.0 ** -8)])
    xd, flat, off = R.carve(x, DEV)
    got = _ext().pad_cast_bf16(xd, kp)
    want = torch.nn.functional.pad(xd, (0, kp - k)).to(BF16)
    assert got.shape == (m, kp) and got.dtype == BF16 and got.is_contiguous()
    assert bool((_bits(got) == _bits(want)).all()), \
        f"{int((_bits(got) != _bits(want)).sum())} elements differ"
    assert bool((_bits(got)[:, k:] == 0).all())
    assert (got[:, :k].float().cpu() != x).float().mean() > 0.5
    assert R.outside_untouched(flat, off, x.numel(), float("nan"))
    assert torch.equal(xd.cpu(), x)
    with pytest.raises(RuntimeError):
        _ext().pad_cast_bf16(xd, k - 1)
    with pytest.raises(RuntimeError):
        _ext().pad_cast_bf16(xd.to(BF16), kp)
