"""dien_aux_fwd / dien_aux_bwd (ops/hip/dien_aux_kernels.hip) and the DIEN
wiring against the fp64 evaluation of
  m = mask[b,t] mask[b,t+1] (perm[b] != b)
  z_x = sigmoid([bf(h[b,t]) | bf(e_x[t+1])] W1^T + b1) . w2 + b2
  loss = sum m (softplus(-z_c) + softplus(z_n)) / sum m      (0 if sum m == 0)
on the same bf16 weights and fp32 inputs (gradients: fp64 autograd, the
rounding of h and seq passed straight through). Operands are carved out of
NaN-filled buffers so that a read past an operand shows.

Yardstick: the bf16 composition the project would otherwise use, on the GPU
with the same operands: FusedLinear(H+Di -> A, sigmoid) -> FusedLinear(A -> 1)
on the concatenated rows (zero rows appended up to a multiple of 16: below
that FusedLinear computes in fp32), BCE and the masked mean in fp32 torch;
rel_l2(fused) <= 2 rel_l2(yardstick) per tensor, the margin of
test_model_fused_against_autocast: both carry the bf16 operand noise, the
fused path rounds neither the hidden activations nor the logits. Observed
ratios are in profiles/PERF_LOG.md ("Fused DIEN auxiliary loss").
"""
import functools
import math

import pytest
import torch

from tests import dense_reference as D
from tests import seq_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, T, H, Di, A): one row per sample; the reference width (ragged K
# padding, 51 rows: a tile straddles samples); the model; H != Di and A not
# a power of two; the limits
SHAPES = [(2, 2, 4, 4, 16), (3, 18, 36, 36, 64), (2, 50, 32, 32, 64),
          (5, 23, 16, 64, 48), (4, 9, 64, 64, 128)]
MASKS = ["prefix", "all", "holes", "dead"]
NAMES = ("loss", "dh", "dseq", "dW1", "db1", "dw2", "db2")
GRAD_OUT = 0.75


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _merge_shape():
    """More than two rounds of four 16-row tiles per workgroup."""
    from deeprec_amd.ops.fused_aux_loss import dien_aux_workgroups
    return (8 * 16 * dien_aux_workgroups(1 << 20) // 17 + 3, 18, 4, 4, 16)


def _mask(b, t, pattern):
    gen = S._gen(b, t, len(pattern), 41)
    m = torch.ones(b, t, dtype=torch.bool)
    if pattern == "prefix":
        m = torch.arange(t)[None] < torch.randint(2, t + 1, (b, 1),
                                                  generator=gen)
    elif pattern == "holes":
        m = torch.rand(b, t, generator=gen) < 0.6
        m[:, :2] = True
        for r in range(16, 32):     # a whole dead tile of flattened rows
            m[r // (t - 1), r % (t - 1)] = False
    elif pattern == "dead":
        m[b // 2] = False
    elif pattern == "none":
        m[:] = False
    return m


def _perm(b):
    """Sample 0 is paired with itself (a dropped pair, and a dnoclick slab
    of zeros), the others go round one random cycle. At B = 2 that would
    leave no live pair at all, so there the two samples are swapped."""
    if b == 2:
        return torch.tensor([1, 0])
    rest = 1 + torch.randperm(b - 1, generator=S._gen(b, 53))
    p = torch.zeros(b, dtype=torch.int64)
    p[rest] = rest.roll(-1)
    return p


def _live(mask, perm):
    paired = (perm != torch.arange(len(perm)))[:, None]
    return mask[:, :-1] & mask[:, 1:] & paired


@functools.lru_cache(maxsize=None)
def _case(b, t, hd, di, a):
    gen = S._gen(b, t, hd, di, a, 43)
    k = hd + di
    return {"h": torch.randn(b, t, hd, generator=gen),
            "seq": torch.randn(b, t, di, generator=gen),
            "w1": S.randn_bf16(gen, a, k, scale=k ** -0.5),
            "b1": 0.1 * torch.randn(a, generator=gen),
            "w2": S.randn_bf16(gen, a, scale=a ** -0.5),
            "b2": 0.1 * torch.randn(1, generator=gen)}


def _loss(h, seq, perm, m, net):
    """The definition on [h_t | e_{t+1}] rows; net: rows -> logits."""
    click = seq[:, 1:]
    rows = torch.stack([torch.cat([h[:, :-1], click], -1),
                        torch.cat([h[:, :-1], click[perm]], -1)])
    z = net(rows.reshape(-1, rows.shape[-1])).reshape(2, *m.shape)
    sp = torch.nn.functional.softplus
    return ((sp(-z[0]) + sp(z[1])) * m).sum() / m.sum().clamp_min(1)


@functools.lru_cache(maxsize=None)
def _ref(shape, pattern):
    c, mask, perm = _case(*shape), _mask(*shape[:2], pattern), _perm(shape[0])
    leaves = [c[k].double().requires_grad_()
              for k in ("h", "seq", "w1", "b1", "w2", "b2")]
    h, seq, w1, b1, w2, b2 = leaves
    h16 = h + (c["h"].to(S.BF16).double() - h).detach()
    s16 = seq + (c["seq"].to(S.BF16).double() - seq).detach()
    loss = _loss(h16, s16, perm, _live(mask, perm).double(),
                 lambda x: torch.sigmoid(x @ w1.t() + b1) @ w2 + b2)
    grads = torch.autograd.grad(loss * GRAD_OUT, leaves)
    return dict(zip(NAMES, (loss.detach(), *grads)))


def _fused(shape, pattern, **over):
    c = dict(_case(*shape), **over)
    mask, perm = _mask(*shape[:2], pattern), _perm(shape[0])
    h, seq, w1, b1, w2, b2 = (
        D.carve(c[k], DEV)[0] for k in ("h", "seq", "w1", "b1", "w2", "b2"))
    # bytes past the mask read as valid steps, entries past perm as bad ones
    mk = D.carve(mask.to(torch.uint8), DEV, fill=1)[0]
    pm = D.carve(perm, DEV, fill=1 << 40)[0]
    loss, msum = _ext().dien_aux_fwd(h, seq, mk, pm, w1, b1, w2, b2)
    got = _ext().dien_aux_bwd(torch.tensor([GRAD_OUT], device=DEV), msum, h,
                              seq, mk, pm, w1, b1, w2, b2)
    res = dict(zip(("loss", "dh", "dclick", "dnoclick") + NAMES[3:],
                   (loss, *got)), dseq=got[1] + got[2])
    return {k: v.cpu() for k, v in res.items()}


def _unfused(shape, pattern, weights=None):
    from deeprec_amd.ops.fused_mlp import FusedLinear
    c, mask, perm = _case(*shape), _mask(*shape[:2], pattern), _perm(shape[0])
    hd, di, a = shape[2:]
    lin1 = FusedLinear(hd + di, a, activation="sigmoid").to(DEV)
    lin2 = FusedLinear(a, 1, activation=None).to(DEV)
    with torch.no_grad():
        lin1.weight.copy_(c["w1"].float())
        lin1.bias.copy_(c["b1"])
        lin2.weight.copy_(c["w2"].float().view(1, a))
        lin2.bias.copy_(c["b2"])
    h = c["h"].to(DEV).requires_grad_()
    seq = c["seq"].to(DEV).requires_grad_()

    def net(x):
        pad = x.new_zeros(-x.shape[0] % 16, x.shape[1])
        return lin2(lin1(torch.cat([x, pad]))).float()[:x.shape[0]]

    loss = _loss(h, seq, perm.to(DEV), _live(mask, perm).float().to(DEV), net)
    (loss * GRAD_OUT).backward()
    res = (loss.detach(), h.grad, seq.grad, lin1.weight.grad, lin1.bias.grad,
           lin2.weight.grad.view(-1), lin2.bias.grad)
    return {k: v.float().cpu() for k, v in zip(NAMES, res)}


def _within_yardstick(tag, got, ref, plain, names=NAMES):
    for name in names:
        fused = S.rel_l2(got[name], ref[name])
        unf = S.rel_l2(plain[name], ref[name])
        print(f"dien_aux {tag} {name}: fused {fused:.3e} unfused {unf:.3e} "
              f"ratio {fused / unf if unf else 0.0:.2f}")
        assert fused <= 2 * unf, name


def _cases():
    for shape in SHAPES:
        for pattern in MASKS:
            if pattern == "holes" and shape[0] * (shape[1] - 1) < 48:
                continue
            yield shape, pattern


@pytest.mark.parametrize("shape,pattern", list(_cases()))
def test_against_fp64_with_the_unfused_yardstick(shape, pattern):
    got = _fused(shape, pattern)
    mask, perm = _mask(*shape[:2], pattern), _perm(shape[0])
    dead = ~_live(mask, perm)
    assert not any(torch.isnan(v).any() for v in got.values())
    assert not got["dh"][:, -1].any() and not got["dseq"][:, 0].any()
    assert not got["dh"][:, :-1][dead].any()
    assert not got["dclick"][:, 1:][dead].any()
    assert not got["dnoclick"][perm][:, 1:][dead].any()
    _within_yardstick(f"{shape} {pattern}", got, _ref(shape, pattern),
                      _unfused(shape, pattern))


def test_zero_output_layer_gives_two_ln2():
    """w2 = 0, b2 = 0: every logit is 0 and every live pair adds
    2 softplus(0) = 2 ln 2. The loss is a sum of n <= B (T - 1) such terms
    over n: at most n additions of half an fp32 ulp of the running sum, plus
    the division and the roundings of expf and log1pf, a few ulp each:
    (n + 16) U32 relative. No gradient reaches the first layer."""
    shape = SHAPES[1]
    a = shape[4]
    got = _fused(shape, "prefix", w2=torch.zeros(a, dtype=S.BF16),
                 b2=torch.zeros(1))
    n = shape[0] * (shape[1] - 1)
    assert abs(float(got["loss"]) - 2 * math.log(2)) <= (
        (n + 16) * S.U32 * 2 * math.log(2))
    for name in ("dh", "dseq", "dW1", "db1"):
        assert not got[name].any(), name
    assert got["dw2"].any() and not torch.isnan(got["dw2"]).any()


@pytest.mark.parametrize("shape,pattern", [(SHAPES[1], "none"),
                                           ((1, 18, 36, 36, 64), "all")])
def test_no_live_pair_is_exactly_zero(shape, pattern):
    """An all-dead mask, and B = 1 (perm = [0]: the only sample is paired
    with itself): loss and every gradient are exact zeros."""
    got = _fused(shape, pattern)
    for name, v in got.items():
        assert not torch.isnan(v).any() and not v.any(), name


def test_merge_shape_and_determinism():
    """More than two rounds per workgroup: the persistent loop and the
    cross-workgroup merge run; two calls give bit-identical loss and dW1."""
    shape = _merge_shape()
    got = _fused(shape, "prefix")
    _within_yardstick("merge", got, _ref(shape, "prefix"),
                      _unfused(shape, "prefix"), NAMES[3:])
    again = _fused(shape, "prefix")
    assert torch.equal(again["loss"], got["loss"])
    assert torch.equal(again["dW1"], got["dW1"])


@pytest.mark.parametrize("bad", ["strided", "H6", "A24", "mismatch", "T1"])
def test_host_checks(bad):
    b, t = 2, 1 if bad == "T1" else 5
    hd, di, a = 6 if bad == "H6" else 8, 8, 24 if bad == "A24" else 16
    h = torch.zeros(b, t, hd, device=DEV)
    if bad == "strided":
        h = torch.zeros(b, t, 2 * hd, device=DEV)[:, :, ::2]
    seq = torch.zeros(b + (bad == "mismatch"), t, di, device=DEV)
    args = (h, seq, torch.ones(b, t, device=DEV, dtype=torch.uint8),
            torch.arange(b, device=DEV),
            torch.zeros(a, hd + di, device=DEV, dtype=S.BF16),
            torch.zeros(a, device=DEV),
            torch.zeros(a, device=DEV, dtype=S.BF16),
            torch.zeros(1, device=DEV))
    with pytest.raises(RuntimeError, match="dien_aux_fwd"):
        _ext().dien_aux_fwd(*args)
    with pytest.raises(RuntimeError, match="dien_aux_bwd"):
        _ext().dien_aux_bwd(torch.ones(1, device=DEV),
                            torch.ones(1, device=DEV), *args)


def _graph_has(fn, name, seen):
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return name in type(fn).__name__ or any(
        _graph_has(nxt, name, seen) for nxt, _ in fn.next_functions)


def test_model_wiring(shape=(6, 9, 8, 8, 64)):
    """_auxiliary_loss of a small DIEN, fused and plain, on the case's
    weights; then one full training step of the fused model."""
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.models.sequence import DIEN
    c, mask, perm = _case(*shape), _mask(*shape[:2], "prefix"), _perm(6)
    kw = dict(device=DEV, embedding_dim=4, item_dim=8, gru_hidden=8,
              att_hidden=16, mlp_sizes=(16,))
    models = {"fused": DIEN(fused_aux_loss=True, **kw), "plain": DIEN(**kw)}
    assert set(models["fused"].state_dict()) == set(
        models["plain"].state_dict())
    got = {}
    for key, model in models.items():
        with torch.no_grad():
            for q, k in zip(model.aux_net.parameters(),
                            ("w1", "b1", "w2", "b2")):
                q.copy_(c[k].float().view_as(q))
        loss = model._auxiliary_loss(c["h"].to(DEV), c["seq"].to(DEV),
                                     mask.float().to(DEV),
                                     perm=perm.to(DEV))
        assert _graph_has(loss.grad_fn, "_DienAuxLoss", set()) == (
            key == "fused")
        (loss * GRAD_OUT).backward()
        grads = [q.grad.cpu() for q in model.aux_net.parameters()]
        got[key] = dict(zip(("loss",) + NAMES[3:],
                            [loss.detach().cpu()] + grads))
        got[key]["dw2"] = got[key]["dw2"].view(-1)
    _within_yardstick("model", got["fused"], _ref(shape, "prefix"),
                      _unfused(shape, "prefix"), ("loss",) + NAMES[3:])
    model = models["fused"]
    model.zero_grad()
    ds = CriteoSyntheticDataset(batch_size=64, seed=31, device=DEV)
    b = ds.next_seq_batch(seq_len=9, item_cardinality=1 << 10)
    out = model.loss_fn(model(b[0], b[1][:, :model.num_sparse], b[2], b[3]),
                        b[4])
    out.backward()
    assert torch.isfinite(out)
    assert all(q.grad is not None for q in model.parameters())
