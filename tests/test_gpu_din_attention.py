"""din_attn_fwd / din_attn_bwd (ops/hip/din_attention_kernels.hip) and the
DIN wiring against the fp64 evaluation of
  f = bf16([s, t, s-t, s*t]); sc = sigmoid(f W1^T + b1) . w2
  w = softmax over the live positions; out = sum_t w[t] s_t
on the same bf16 weights and fp32 inputs (gradients: fp64 autograd, the
rounding of f passed straight through). Operands are carved out of
NaN-filled buffers so that a read past an operand shows.

Yardstick: today's unfused GPU composition (din_att_features -> FusedLinear
-> FusedLinear -> masked_softmax_pool) on the same operands;
rel_l2(fused) <= 2 rel_l2(unfused) per tensor, the margin of
test_model_fused_against_autocast: both carry the bf16 operand noise, the
fused path rounds neither h nor the scores. Observed ratios are in
profiles/PERF_LOG.md ("Fused DIN attention").
"""
import functools
import gc

import pytest
import torch

from tests import dense_reference as D
from tests import seq_reference as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, T, D, H): smallest; partial second tile at the model's widths; the
# model's T; a wave's second tile and H not a power of two; widest W1
SHAPES = [(1, 1, 8, 16), (3, 17, 32, 64), (2, 50, 32, 64), (5, 70, 16, 48),
          (4, 33, 64, 128)]
MASKS = ["prefix", "all", "holes", "dead"]
NAMES = ("out", "dseq", "dtgt", "dW1", "db1", "dw2")


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _merge_shape():
    from deeprec_amd.ops.fused_attention import din_attention_workgroups
    return (2 * din_attention_workgroups(1 << 20) + 3, 3, 8, 16)


def _mask(b, t, pattern):
    gen = S._gen(b, t, len(pattern), 41)
    m = torch.ones(b, t, dtype=torch.bool)
    if pattern == "prefix":
        m = torch.arange(t)[None] < torch.randint(1, t + 1, (b, 1),
                                                  generator=gen)
    elif pattern == "holes":
        m = torch.rand(b, t, generator=gen) < 0.6
        m[:, 16:32] = False     # a whole dead tile in the middle
        m[:, 0] = True
    elif pattern == "dead":
        m[b // 2] = False
    return m


@functools.lru_cache(maxsize=None)
def _case(b, t, d, h):
    gen = S._gen(b, t, d, h, 43)
    k = 4 * d
    return {"seq": S.randn_bf16(gen, b, t, d).float(),
            "tgt": S.randn_bf16(gen, b, d).float(),
            "dout": S.randn_bf16(gen, b, d).float(),
            "w1": S.randn_bf16(gen, h, k, scale=k ** -0.5),
            "b1": 0.1 * torch.randn(h, generator=gen),
            "w2": S.randn_bf16(gen, h, scale=h ** -0.5)}


def _features(seq, tgt):
    t = tgt[:, None, :].expand_as(seq)
    return torch.cat([seq, t, seq - t, seq * t], 2)


@functools.lru_cache(maxsize=None)
def _ref(shape, pattern):
    c, mask = _case(*shape), _mask(shape[0], shape[1], pattern)
    leaves = [c[k].double().requires_grad_()
              for k in ("seq", "tgt", "w1", "b1", "w2")]
    seq, tgt, w1, b1, w2 = leaves
    f = _features(seq, tgt)
    f16 = _features(c["seq"], c["tgt"]).to(S.BF16).double()
    f = f + (f16 - f).detach()
    sc = torch.sigmoid(f @ w1.t() + b1) @ w2
    mx = sc.masked_fill(~mask, -torch.inf).amax(1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(sc - mx) * mask
    w = e / e.sum(1, keepdim=True).clamp_min(1e-300)
    out = (w[:, :, None] * seq).sum(1)
    grads = torch.autograd.grad((out * c["dout"].double()).sum(), leaves)
    return dict(zip(NAMES, (out.detach(), *grads)), w=w.detach())


def _fused(shape, pattern):
    c, mask = _case(*shape), _mask(shape[0], shape[1], pattern)
    seq, tgt, dout, w1, b1, w2 = (
        D.carve(c[k], DEV)[0] for k in ("seq", "tgt", "dout", "w1", "b1",
                                        "w2"))
    # bytes past the mask read as live positions
    mk = D.carve(mask.to(torch.uint8), DEV, fill=1)[0]
    out, w = _ext().din_attn_fwd(seq, tgt, mk, w1, b1, w2)
    got = _ext().din_attn_bwd(dout, seq, tgt, mk, w, w1, b1, w2)
    res = dict(zip(NAMES, (out, *got[:5])), db2=got[5], w=w)
    return {k: v.cpu() for k, v in res.items()}


def _unfused(shape, pattern, dev=DEV):
    from deeprec_amd.ops.fused_attention import (din_att_features,
                                                 masked_softmax_pool)
    from deeprec_amd.ops.fused_mlp import FusedLinear
    c, mask = _case(*shape), _mask(shape[0], shape[1], pattern)
    b, t, d, h = shape
    lin1 = FusedLinear(4 * d, h, activation="sigmoid").to(dev)
    lin2 = FusedLinear(h, 1, activation=None).to(dev)
    with torch.no_grad():
        lin1.weight.copy_(c["w1"].float())
        lin1.bias.copy_(c["b1"])
        lin2.weight.copy_(c["w2"].float().view(1, h))
    seq = c["seq"].to(dev).clone().requires_grad_()
    tgt = c["tgt"].to(dev).clone().requires_grad_()
    scores = lin2(lin1(din_att_features(seq, tgt))).float().reshape(b, t)
    out = masked_softmax_pool(scores, seq, mask.to(dev))
    out.backward(c["dout"].to(dev))
    res = (out.detach(), seq.grad, tgt.grad, lin1.weight.grad,
           lin1.bias.grad, lin2.weight.grad.view(-1))
    return {k: v.float().cpu() for k, v in zip(NAMES, res)}


def _cases():
    for shape in SHAPES:
        for pattern in MASKS:
            if (pattern == "holes" and shape[1] < 33
                    or pattern == "dead" and shape[0] < 2
                    or shape[1] == 1 and pattern != "all"):
                continue
            yield shape, pattern


@pytest.mark.parametrize("shape,pattern", list(_cases())[1:])
def test_against_fp64_with_the_unfused_yardstick(shape, pattern):
    ref, got = _ref(shape, pattern), _fused(shape, pattern)
    plain = _unfused(shape, pattern)
    mask = _mask(shape[0], shape[1], pattern)
    assert not any(torch.isnan(v).any() for v in got.values())
    assert torch.equal(got["db2"], torch.zeros(1))
    assert bool((got["w"][~mask] == 0).all())
    for b in (~mask.any(1)).nonzero().flatten().tolist():
        assert not got["out"][b].any() and not got["dseq"][b].any()
        assert not got["dtgt"][b].any()
    for name in NAMES:
        fused = S.rel_l2(got[name], ref[name])
        unf = S.rel_l2(plain[name], ref[name])
        print(f"din_attention {shape} {pattern} {name}: fused {fused:.3e} "
              f"unfused {unf:.3e} ratio {fused / unf:.2f}")
        assert fused <= 2 * unf, name


def test_one_live_position_is_exact():
    """(1, 1, 8, 16): w == 1, out == seq[0, 0], dseq == dout; every other
    gradient is zero in fp64 by cancellation of dout.s - w dout.s, so the
    bound is the rounding of those two equal terms, 4 U32 |dout.s|, times
    the largest factor it multiplies. The unfused composition on the CPU
    meets the same bound."""
    shape = SHAPES[0]
    c, got = _case(*shape), _fused(shape, "all")
    assert torch.equal(got["w"], torch.ones(1, 1))
    assert torch.equal(got["out"], c["seq"][0])
    assert torch.equal(got["dseq"], c["dout"][:, None, :])
    assert torch.equal(got["db2"], torch.zeros(1))
    f = _features(c["seq"], c["tgt"]).abs().max()
    factor = max(1.0, float(c["w2"].float().abs().max())) * max(
        1.0, float(f), float(c["w1"].float().abs().max()))
    bound = 4 * S.U32 * abs(float((c["dout"] * c["seq"][0]).sum())) * factor
    cpu = _unfused(shape, "all", dev="cpu")
    for name in ("dtgt", "dW1", "db1", "dw2"):
        assert float(cpu[name].abs().max()) <= bound, name
        assert float(got[name].abs().max()) <= bound, name


def test_merge_shape_and_determinism():
    """More samples than twice the workgroups: the persistent loop and the
    cross-workgroup merge run; two calls give bit-identical dW1."""
    shape = _merge_shape()
    ref, got = _ref(shape, "prefix"), _fused(shape, "prefix")
    plain = _unfused(shape, "prefix")
    for name in NAMES[1:]:
        fused = S.rel_l2(got[name], ref[name])
        unf = S.rel_l2(plain[name], ref[name])
        print(f"din_attention merge {name}: fused {fused:.3e} unfused "
              f"{unf:.3e} ratio {fused / unf:.2f}")
        assert fused <= 2 * unf, name
    assert torch.equal(_fused(shape, "prefix")["dW1"], got["dW1"])


@pytest.mark.parametrize("bad", ["strided", "D12", "H24", "mismatch"])
def test_host_checks(bad):
    b, t, d, h = 2, 5, 12 if bad == "D12" else 8, 24 if bad == "H24" else 16
    seq = torch.zeros(b, t, d, device=DEV)
    if bad == "strided":
        seq = torch.zeros(b, t, 2 * d, device=DEV)[:, :, ::2]
    tgt = torch.zeros(b + (bad == "mismatch"), d, device=DEV)
    mask = torch.ones(b, t, device=DEV, dtype=torch.uint8)
    w1 = torch.zeros(h, 4 * d, device=DEV, dtype=S.BF16)
    b1 = torch.zeros(h, device=DEV)
    w2 = torch.zeros(h, device=DEV, dtype=S.BF16)
    with pytest.raises(RuntimeError, match="din_attn_fwd"):
        _ext().din_attn_fwd(seq, tgt, mask, w1, b1, w2)
    with pytest.raises(RuntimeError, match="din_attn_bwd"):
        _ext().din_attn_bwd(torch.zeros(b, d, device=DEV), seq, tgt, mask,
                            torch.zeros(b, t, device=DEV), w1, b1, w2)


def _graph_has(fn, name, seen):
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return name in type(fn).__name__ or any(
        _graph_has(nxt, name, seen) for nxt, _ in fn.next_functions)


@pytest.mark.parametrize("flat_ws", [False, True])
def test_model_fused_against_unfused(flat_ws, batch=32, t=9):
    """Logits and the att.* gradients of a small DIN, fused and unfused,
    each against the fp64 CPU model on the same weights and inputs.
    flat_ws: the att layers' dw_ws slices are set by hand and the fused
    gradients have to land in them."""
    from deeprec_amd.models.sequence import DIN
    gen = S._gen(batch, t, 47)
    kw = dict(embedding_dim=4, item_dim=8, att_hidden=16, mlp_sizes=(16,))
    emb = S.randn_bf16(gen, batch, 10, 4).double()
    seq = S.randn_bf16(gen, batch, t, 8).double()
    tgt = S.randn_bf16(gen, batch, 8).double()
    dense = S.randn_bf16(gen, batch, 13).double()
    seq_ids = (_mask(batch, t, "prefix")).long()
    labels = (torch.rand(batch, generator=gen) < 0.5).double()

    class Ref64(DIN):
        compute_dtype = torch.float64   # the fp32 debug path, in fp64

    torch.manual_seed(0)
    models = {"ref": Ref64(device="cpu", bf16=False, **kw).double(),
              "fused": DIN(device=DEV, fused_attention=True, **kw),
              "plain": DIN(device=DEV, **kw)}
    assert set(models["fused"].state_dict()) == set(
        models["plain"].state_dict())
    res, slices = {}, None
    for key, model in models.items():
        with torch.no_grad():
            for q, src in zip(model.parameters(),
                              models["ref"].parameters()):
                q.copy_(src)
        dev = model.device_
        dt = next(model.parameters()).dtype
        model.sparse_feats = lambda ids, train=True, d=dev: emb.to(d, dt)
        model.seq_and_target = lambda s, g, train=True, d=dev: (
            seq.to(d, dt), tgt.to(d, dt))
        if flat_ws and key == "fused":
            slices = [torch.full((m.weight.numel() + m.bias.numel(),),
                                 float("nan"), device=DEV) for m in model.att]
            for m, ws in zip(model.att, slices):
                m.dw_ws = ws
        logits = model(dense.to(dev, dt), None, seq_ids.to(dev), None)
        assert _graph_has(logits.grad_fn, "_DinAttention", set()) == (
            key == "fused")
        torch.nn.functional.binary_cross_entropy_with_logits(
            logits.double(), labels.to(dev)).backward()
        att = [q for n, q in model.named_parameters() if n.startswith("att.")]
        res[key] = [logits.detach().cpu().double()] + [
            q.grad.detach().cpu().double() for q in att]
    if flat_ws:
        for m, ws in zip(models["fused"].att, slices):
            n = m.weight.numel()
            assert torch.equal(ws[:n].view_as(m.weight), m.weight.grad)
            assert torch.equal(ws[n:], m.bias.grad)
    names = ["logits", "att.0.weight", "att.0.bias", "att.1.weight"]
    for name, ref, fused, plain in zip(names, res["ref"], res["fused"],
                                       res["plain"]):
        a, b = S.rel_l2(fused, ref), S.rel_l2(plain, ref)
        print(f"din {name}: fused {a:.3e} unfused {b:.3e} ratio {a / b:.2f}")
        assert a <= 2 * b, name
    assert not res["fused"][4].any()    # att.1.bias: db2 is exactly zero


def _seq_loss(model, dense, ids, seq, target, labels):
    logits = model(dense, ids[:, :model.num_sparse], seq, target)
    return model.loss_fn(logits, labels)


def test_captured_fused_din_matches_eager():
    """A static_seq, fused_attention DIN captured by GraphedTrainStep and
    replayed for three steps against an eager twin: the losses agree to
    one bf16 ulp of the largest logit (the bound of
    test_bench_captured_dump_independent_of_steps)."""
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    from deeprec_amd.models.sequence import DIN
    from deeprec_amd.optimizers import AdamAsyncOptimizer
    from deeprec_amd.training.graph_step import GraphedTrainStep
    ds = CriteoSyntheticDataset(batch_size=256, seed=31, device=DEV)
    batches = [ds.next_seq_batch(seq_len=20, item_cardinality=1 << 12)
               for _ in range(4)]

    def make():
        torch.manual_seed(5)
        m = DIN(device=DEV, bf16=True, static_seq=True, fused_attention=True,
                ev_option=EmbeddingVariableOption(init_capacity=1 << 14))
        o = AdamAsyncOptimizer(params=m.parameters(),
                               embedding_variables=m.embedding_variables(),
                               learning_rate=0.001, graph_safe=True)
        return m, o

    mg, og = make()
    step = GraphedTrainStep(mg, og, _seq_loss, batches[0],
                            expected_entries=1 << 16, expected_slots=1 << 16)
    assert step.graph is not None, "capture must succeed"
    graphed = [float(step(b).detach()) for b in batches[1:]]
    me, oe = make()
    eager, top = [], 0.0
    for i, b in enumerate([batches[0], batches[0]] + batches[1:]):
        logits = me(b[0], b[1][:, :me.num_sparse], b[2], b[3])
        le = me.loss_fn(logits, b[4])
        oe.zero_grad()
        le.backward()
        oe.step()
        if i >= 2:
            eager.append(float(le))
            top = max(top, float(logits.abs().max()))
    torch.cuda.synchronize()
    print("losses graphed", graphed, "eager", eager, "ulp", 2.0 ** -7 * top)
    for a, b in zip(graphed, eager):
        assert abs(a - b) <= 2.0 ** -7 * top
    step.graph = None
    del step
    gc.collect()
    torch.cuda.synchronize()
