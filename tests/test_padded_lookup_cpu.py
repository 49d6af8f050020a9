"""embedding_lookup(pad_id=...) and static_seq sequence models on CPU.

The padded lookup must be indistinguishable from "drop the pads, look the
rest up, scatter into zeros" — in its output and in everything it leaves
in the table."""
import pytest
import torch

from deeprec_amd.embedding import EmbeddingVariable, embedding_lookup
from deeprec_amd.optimizers import GradientDescentOptimizer

DIM = 6


def _ev(seed):
    return EmbeddingVariable("items", DIM, device="cpu",
                             generator=torch.Generator().manual_seed(seed))


def _masked_reference(ev, ids, pad_id):
    """zeros + a plain lookup of the non-pad ids (the oracle)."""
    flat = ids.reshape(-1)
    keep = flat != pad_id
    out = torch.zeros(flat.numel(), ev.dim)
    if bool(keep.any()):
        out = out.index_put((keep.nonzero().squeeze(1),),
                            embedding_lookup(ev, flat[keep]))
    return out.reshape(*ids.shape, ev.dim)


def _sorted_export(ev):
    keys, values, freqs, versions = ev.export()
    o = torch.argsort(keys)
    return keys[o], values[o], freqs[o], versions[o]


def _fill(shape, pad_id, kind):
    """ids of `shape` for one pad pattern; valid ids avoid pad_id."""
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator().manual_seed(n * 7 + 1)
    valid = torch.randint(1, 50, (n,), generator=g)
    if pad_id == -1:
        valid[0] = 0  # 0 is an ordinary id when the pad id is -1
    pad = torch.full((n,), pad_id, dtype=torch.int64)
    if kind == "none":
        flat = valid
    elif kind == "all":
        flat = pad
    elif kind == "single":
        flat = pad.clone()
        flat[n // 2] = valid[n // 2]
    elif kind == "repeat":
        # one valid id repeated, pads on both sides of each occurrence
        flat = pad.clone()
        flat[1::2] = 17
    else:  # mixed
        flat = torch.where(torch.rand(n, generator=g) < 0.5, pad, valid)
    return flat.reshape(shape)


@pytest.mark.parametrize("pad_id", [0, -1])
@pytest.mark.parametrize("shape", [(7,), (5, 4), (3, 2, 3)])
@pytest.mark.parametrize("kind", ["none", "all", "single", "repeat", "mixed"])
def test_padded_lookup_matches_masked_reference(pad_id, shape, kind):
    ids = _fill(shape, pad_id, kind)
    ev, twin = _ev(5), _ev(5)
    assert torch.equal(ev.storage.default_values,
                       twin.storage.default_values)
    opt = GradientDescentOptimizer(embedding_variables=[ev],
                                   learning_rate=0.5)
    opt_t = GradientDescentOptimizer(embedding_variables=[twin],
                                     learning_rate=0.5)
    w = torch.randn(*shape, DIM, generator=torch.Generator().manual_seed(2))

    out = embedding_lookup(ev, ids, pad_id=pad_id)
    ref = _masked_reference(twin, ids, pad_id)
    assert out.shape == (*shape, DIM)
    assert torch.equal(out, ref)
    assert torch.equal(out[ids == pad_id],
                       torch.zeros_like(out[ids == pad_id]))

    for o, e, op in ((out, ev, opt), (ref, twin, opt_t)):
        op.zero_grad()
        if o.requires_grad:
            (o * w).sum().backward()
        op.step(increment_global_step=False)
    ke, ve, fe, _ = _sorted_export(ev)
    kt, vt, ft, _ = _sorted_export(twin)
    assert torch.equal(ke, kt)
    assert torch.equal(ve, vt)
    assert torch.equal(fe, ft)
    assert ev.size() == twin.size()
    valid = ids[ids != pad_id]
    assert ev.size() == torch.unique(valid).numel()
    assert not bool((ke == pad_id).any())


def test_padded_lookup_inference_inserts_nothing():
    ev = _ev(3)
    ids = torch.tensor([[4, 0, 9], [0, 0, 4]])
    embedding_lookup(ev, ids[:, :1], pad_id=0)  # admits key 4 only
    out = embedding_lookup(ev, ids, train=False, pad_id=0)
    assert ev.size() == 1
    assert torch.equal(out[ids == 0], torch.zeros(3, DIM))
    assert torch.equal(out[0, 0], out[1, 2])


def test_padded_lookup_records_no_pad():
    ev = _ev(3)
    ev.start_sparse_recording()
    embedding_lookup(ev, torch.tensor([0, 8, 0, 3, 8]), pad_id=0)
    assert ev.consume_recorded_ids().tolist() == [3, 8]


# ---------------------------------------------------------------- models

def _seq_batch(b=6, t=5):
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    ds = CriteoSyntheticDataset(batch_size=b, seed=9)
    dense, ids, seq, target, labels = ds.next_seq_batch(seq_len=t)
    seq[2] = 0                  # one row with an empty history
    target[0] = seq[0, 0]       # a key the sequence and the target share
    return dense, ids, seq, target, labels


@pytest.mark.parametrize("name", ["din", "bst", "dien"])
def test_static_seq_model_matches_masked(name):
    from deeprec_amd.models import MODEL_REGISTRY
    dense, ids, seq, target, labels = _seq_batch()
    assert int((seq[2] != 0).sum()) == 0 and int((seq == 0).sum()) > 5
    kw = dict(use_aux_loss=True) if name == "dien" else {}
    logits, exports = [], []
    for static in (False, True):
        torch.manual_seed(0)
        m = MODEL_REGISTRY[name](device="cpu", bf16=False,
                                 static_seq=static, **kw)
        assert m.static_seq is static
        opt = GradientDescentOptimizer(
            params=m.parameters(),
            embedding_variables=m.embedding_variables(), learning_rate=0.1)
        torch.manual_seed(1)    # DIEN's aux loss draws a permutation
        out = m(dense, ids[:, :m.num_sparse], seq, target)
        loss = m.loss_fn(out, labels)
        opt.zero_grad()
        loss.backward()
        opt.step(increment_global_step=False)
        logits.append(out.detach())
        exports.append(_sorted_export(m.item_ev))
    assert torch.equal(logits[0], logits[1])
    (k0, v0, f0, ver0), (k1, v1, f1, ver1) = exports
    assert torch.equal(k0, k1)
    assert not bool((k0 == 0).any())
    assert torch.equal(f0, f1)
    assert torch.equal(ver0, ver1)
    # the shared key takes two SGD applies on the masked path and one
    # apply of the summed gradient on the fused path: fp32 reassociation
    # of w - lr*g1 - lr*g2, a few ulp of values of magnitude < 1
    torch.testing.assert_close(v0, v1, rtol=0, atol=1e-6)
