"""Static-shape padded sequence lookup on the HIP engine: the pad-aware
gather, the padded dedup with its CSR order, embedding_lookup(pad_id=...)
eager and captured, and the captured DIN/BST training step.

Comparisons are exact wherever the arithmetic allows: the gather is a
copy, dedup outputs are integers, and the backward runs on integer-valued
gradients in [-8, 8] whose fp32 sums are exact in any order (with SGD at
lr 0.5 the product is exact too), so atomic order cannot show."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD_KEY = 2 ** 63 - 1


# --------------------------------------------------------------------------
# seq_gather_pad
# --------------------------------------------------------------------------

def _gather_case(nnz, dim, share, gen):
    """A padded (keys, slots) pair with a -1 tail and some unadmitted
    rows, and an inverse with the given share of pads."""
    n_u = min(nnz, 37)
    tail = 9
    n_slots, dvd = 64, 5
    values = torch.randn(n_slots, dim, generator=gen)
    default_values = torch.randn(dvd, dim, generator=gen)
    keys = torch.randint(0, 1 << 40, (n_u + tail,), generator=gen)
    slots = torch.randint(0, n_slots, (n_u + tail,), generator=gen,
                          dtype=torch.int32)
    slots[::5] = -1                 # known key without a value row
    keys[n_u:] = PAD_KEY            # capture tail: never referenced
    slots[n_u:] = -1
    inverse = torch.randint(0, n_u, (nnz,), generator=gen, dtype=torch.int32)
    if share == "half":
        inverse[torch.rand(nnz, generator=gen) < 0.5] = -1
    elif share == "all":
        inverse[:] = -1
    elif share == "all_but_one":
        keep = int(inverse[nnz // 2])
        inverse[:] = -1
        inverse[nnz // 2] = keep
    return values, default_values, keys, slots, inverse


def _gather_reference(values, default_values, keys, slots, inverse, npv,
                      use_np, dtype):
    rows = default_values[keys % default_values.shape[0]]
    if use_np:
        rows = torch.full_like(rows, npv)
    has = slots >= 0
    rows[has] = values[slots[has].long()]
    out = torch.zeros(inverse.numel(), values.shape[1])
    valid = inverse >= 0
    out[valid] = rows[inverse[valid].long()]
    return out.to(dtype)            # torch's own rounding for bf16


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim", [1, 3, 16, 32, 130])
def test_seq_gather_pad_is_a_copy(dim, dtype):
    from deeprec_amd.ops.build_ext import require_extension
    ext = require_extension()
    gen = torch.Generator().manual_seed(dim)
    for nnz in (1, 63, 65, 257, 2049):
        for share in ("none", "half", "all", "all_but_one"):
            case = _gather_case(nnz, dim, share, gen)
            dev = [t.to(DEV) for t in case]
            for use_np in (False, True):
                out = ext.seq_gather_pad(*dev, -0.75, use_np, dtype)
                ref = _gather_reference(*case, -0.75, use_np, dtype)
                assert out.shape == (nnz, dim) and out.dtype == dtype
                assert torch.equal(out.cpu(), ref), (nnz, share, use_np)


# --------------------------------------------------------------------------
# padded dedup + CSR order + segmented backward
# --------------------------------------------------------------------------

def _storage(graph):
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    from deeprec_amd.ops.hip_backend import HbmStorage
    st = HbmStorage(8, EmbeddingVariableOption(init_capacity=8192),
                    device=DEV, generator=torch.Generator().manual_seed(5))
    if graph:
        st.enable_graph_mode(4096, 4096)
    return st


def _padded_stream(nnz, stream, gen):
    """keys with about a third of pads (at least one valid position)."""
    keys = (torch.randperm(4 * nnz + 8, generator=gen)[:nnz] + 1000).long()
    pad = torch.rand(nnz, generator=gen) < 0.34
    pad[nnz // 2] = False
    if stream == "hot":
        # one key on 90 % of the valid positions: its run in `order` is
        # far longer than the backward's groups of 8 occurrences
        hot = (torch.rand(nnz, generator=gen) < 0.9) & ~pad
        keys[hot] = 777
    keys[pad] = PAD_KEY
    return keys


def _check_padded_dedup(st, keys, graph):
    nnz = keys.numel()
    kd = keys.to(DEV)
    e0 = int(st.entry_counter)
    if graph:
        d = st.dedup_lookup_capture(kd, pad=True)
        m = int(d.m_dev)
    else:
        d = st.dedup_lookup(kd, 1, pad=True)
        m = d.uniq.numel()
    mp = d.counts.numel()
    bounds = torch.zeros(mp + 1, dtype=torch.int32, device=DEV)
    bounds[1:] = d.counts.cumsum(0)
    order = st.ext.csr_scatter_pad(d.inverse, d.rank, bounds, st.error_flag)
    st._check_error()
    grew = int(st.entry_counter) - e0

    uniq, inv, cnt, rank, slots, order, bounds = (
        t.cpu() for t in (d.uniq, d.inverse, d.counts, d.rank, d.slots,
                          order, bounds))
    valid = keys != PAD_KEY
    vidx = valid.nonzero().squeeze(1)
    n_valid = vidx.numel()
    ref_u, ref_c = torch.unique(keys[valid], return_counts=True)
    assert m == ref_u.numel()
    su, so = torch.sort(uniq[:m])
    assert torch.equal(su, ref_u)
    assert torch.equal(cnt[:m][so].long(), ref_c)
    assert torch.equal(uniq[inv[valid].long()], keys[valid])
    assert bool((inv[~valid] == -1).all())
    # ranks of a key are a permutation of 0..count-1 <=> bounds + rank
    # enumerates 0..n_valid-1 exactly once
    pos = bounds[inv[valid].long()].long() + rank[valid].long()
    assert bool((rank[valid] >= 0).all())
    assert bool((rank[valid].long() < cnt[inv[valid].long()].long()).all())
    assert torch.equal(torch.sort(pos)[0], torch.arange(n_valid))
    # order: the valid occurrences, grouped by unique row, then -1
    assert torch.equal(torch.sort(order[:n_valid].long())[0], vidx)
    assert torch.equal(
        inv[order[:n_valid].long()].long(),
        torch.repeat_interleave(torch.arange(m), cnt[:m].long()))
    assert bool((order[n_valid:] == -1).all())
    assert bool((slots[:m] >= 0).all())
    if graph:
        assert mp == nnz and bool((slots[m:] == -1).all())
    # the pad never became a table entry
    s, e = st.ext.ht_lookup(torch.tensor([PAD_KEY], device=DEV),
                            st.ht_keys, st.ht_slot, True)
    assert int(s) == -1 and int(e) == -1
    # segmented backward over the pad-aware order, exact on integers
    dim = st.dim
    g = torch.randint(-8, 9, (nnz, dim),
                      generator=torch.Generator().manual_seed(nnz)).float()
    none = torch.Tensor()
    gu = st.ext.group_pooled_bwd_seg(g.to(DEV), order.to(DEV), d.inverse,
                                     none, none, none, mp, nnz, 1, dim,
                                     True, 0).cpu()
    ref = torch.zeros(mp, dim)
    ref.index_add_(0, inv[valid].long(), g[valid])
    assert torch.equal(gu, ref)
    return grew, m


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "capture"])
@pytest.mark.parametrize("stream", ["distinct", "hot"])
@pytest.mark.parametrize("nnz", [1, 65, 257, 2049])
def test_padded_dedup(nnz, stream, graph):
    st = _storage(graph)
    keys = _padded_stream(nnz, stream, torch.Generator().manual_seed(nnz))
    grew, m = _check_padded_dedup(st, keys, graph)
    assert grew == m            # every valid key was new, the pad is none
    grew, _ = _check_padded_dedup(st, keys, graph)
    assert grew == 0            # a fresh epoch over known keys
    assert st.size() == m


def test_padded_dedup_all_pads():
    for graph in (False, True):
        st = _storage(graph)
        kd = torch.full((130,), PAD_KEY, dtype=torch.int64, device=DEV)
        d = (st.dedup_lookup_capture(kd, pad=True) if graph
             else st.dedup_lookup(kd, 1, pad=True))
        mp = d.counts.numel()
        bounds = torch.zeros(mp + 1, dtype=torch.int32, device=DEV)
        bounds[1:] = d.counts.cumsum(0)
        order = st.ext.csr_scatter_pad(d.inverse, d.rank, bounds,
                                       st.error_flag)
        st._check_error()
        assert bool((d.inverse == -1).all()) and bool((order == -1).all())
        assert int(st.entry_counter) == 0 and st.size() == 0
        assert (int(d.m_dev) if graph else d.uniq.numel()) == 0


# --------------------------------------------------------------------------
# the op: against a CPU twin, and captured against an eager twin
# --------------------------------------------------------------------------

DIM = 12


def _ev(device, seed=7):
    from deeprec_amd.embedding import EmbeddingVariable
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    return EmbeddingVariable(
        "items", DIM, device=device,
        ev_option=EmbeddingVariableOption(init_capacity=4096),
        generator=torch.Generator().manual_seed(seed))


def _sgd(ev):
    from deeprec_amd.optimizers import GradientDescentOptimizer
    return GradientDescentOptimizer(embedding_variables=[ev],
                                    learning_rate=0.5)


def _sorted_export(ev):
    keys, values, freqs, versions = (t.cpu() for t in ev.export())
    o = torch.argsort(keys)
    return keys[o], values[o], freqs[o], versions[o]


def _id_batches(shape, gen):
    """all pads, no pads, mixed — ids from a small pool so keys repeat
    within and across batches."""
    full = torch.randint(1, 60, shape, generator=gen)
    mixed = torch.randint(1, 60, shape, generator=gen)
    mixed[torch.rand(shape, generator=gen) < 0.5] = 0
    return [torch.zeros(shape, dtype=torch.int64), full, mixed]


def _int_grad(shape, gen):
    return torch.randint(-8, 9, (*shape, DIM), generator=gen).float()


def test_padded_lookup_matches_cpu_twin():
    from deeprec_amd.embedding import embedding_lookup
    from deeprec_amd.embedding.variable import GLOBAL_STEP
    gen = torch.Generator().manual_seed(3)
    shape = (33, 9)
    evg, evc = _ev(DEV), _ev("cpu")
    assert torch.equal(evg.storage.default_values.cpu(),
                       evc.storage.default_values)
    og, oc = _sgd(evg), _sgd(evc)
    mixed2 = torch.randint(0, 60, shape, generator=gen)
    for step, ids in enumerate(_id_batches(shape, gen)[::-1] + [mixed2]):
        GLOBAL_STEP.value = step + 1
        up = _int_grad(shape, gen)
        outs = []
        for ev, opt, dev in ((evg, og, DEV), (evc, oc, "cpu")):
            out = embedding_lookup(ev, ids.to(dev), pad_id=0)
            opt.zero_grad()
            if out.requires_grad:
                (out * up.to(dev)).sum().backward()
            opt.step(increment_global_step=False)
            outs.append(out.detach().cpu())
        assert outs[0].shape == (*shape, DIM)
        assert torch.equal(outs[0], outs[1]), step
        # inference form: static shape, same rows, inserts nothing
        inf = embedding_lookup(evg, ids.to(DEV), train=False, pad_id=0)
        ref = embedding_lookup(evc, ids, train=False, pad_id=0)
        assert torch.equal(inf.cpu(), ref)
    evg.storage._check_error()
    for a, b in zip(_sorted_export(evg), _sorted_export(evc)):
        assert torch.equal(a, b)
    assert evg.size() == evc.size()
    assert not bool((_sorted_export(evg)[0] == 0).any())


@pytest.mark.parametrize("mode", ["pad", "pad_twice", "plain"])
def test_padded_lookup_captured_matches_eager(mode):
    """Capture lookup + backward + SGD of a graph-mode EV, replay on fresh
    ids, compare with an eager twin fed the batches the graph actually
    ran (capture records, it does not execute). `pad_twice` looks the EV
    up twice per step: its versions must still advance once per step.
    `plain` is the unpadded lookup of a graph-mode EV."""
    from deeprec_amd.embedding import embedding_lookup
    from deeprec_amd.embedding.variable import GLOBAL_STEP
    gen = torch.Generator().manual_seed(17)
    shape = (21, 7)
    pad_id = None if mode == "plain" else 0
    warm = torch.randint(0, 60, shape, generator=gen)
    batches = _id_batches(shape, gen)
    ups = [_int_grad(shape, gen).to(DEV) for _ in range(2)]

    def train_step(ev, opt, ids):
        out = embedding_lookup(ev, ids, pad_id=pad_id)
        loss = (out * ups[0]).sum()
        if mode == "pad_twice":
            out2 = embedding_lookup(ev, ids.flip(0), pad_id=pad_id)
            loss = loss + (out2 * ups[1]).sum()
        opt.zero_grad()
        loss.backward()
        opt.step(increment_global_step=False)

    evg, eve = _ev(DEV), _ev(DEV)
    og, oe = _sgd(evg), _sgd(eve)
    assert GLOBAL_STEP.value == 0
    evg.storage.enable_graph_mode(4096, 4096)   # device step starts at 0
    evg.graph_mode = True
    train_step(evg, og, warm.to(DEV))           # executes: device step 1
    torch.cuda.synchronize()
    static_ids = warm.to(DEV).clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        train_step(evg, og, static_ids)
    torch.cuda.synchronize()
    for ids in batches:                          # device steps 2, 3, 4
        static_ids.copy_(ids)
        g.replay()
    torch.cuda.synchronize()
    evg.storage._check_error()

    for step, ids in enumerate([warm] + batches):
        GLOBAL_STEP.value = step + 1
        train_step(eve, oe, ids.to(DEV))
    torch.cuda.synchronize()
    eve.storage._check_error()

    kg, vg, fg, verg = _sorted_export(evg)
    ke, ve, fe, vere = _sorted_export(eve)
    assert torch.equal(kg, ke)
    assert torch.equal(fg, fe)
    assert torch.equal(verg, vere)
    assert torch.equal(vg, ve)
    if pad_id is not None:
        assert not bool((kg == 0).any())
    g = None
    gc.collect()
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# captured DIN / BST
# --------------------------------------------------------------------------

def _seq_loss(model, dense, ids, seq, target, labels):
    logits = model(dense, ids[:, :model.num_sparse], seq, target)
    return model.loss_fn(logits, labels)


@pytest.mark.parametrize("name", ["din", "bst"])
def test_captured_static_seq_model_matches_eager(name):
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.embedding.options import EmbeddingVariableOption
    from deeprec_amd.models import MODEL_REGISTRY
    from deeprec_amd.optimizers import AdamAsyncOptimizer
    from deeprec_amd.training.graph_step import GraphedTrainStep

    ds = CriteoSyntheticDataset(batch_size=256, seed=31, device=DEV)
    batches = [ds.next_seq_batch(seq_len=8, item_cardinality=1 << 12)
               for _ in range(7)]

    def make():
        torch.manual_seed(5)
        m = MODEL_REGISTRY[name](
            device=DEV, bf16=True, static_seq=True,
            ev_option=EmbeddingVariableOption(init_capacity=1 << 14))
        o = AdamAsyncOptimizer(params=m.parameters(),
                               embedding_variables=m.embedding_variables(),
                               learning_rate=0.001, graph_safe=True)
        return m, o

    mg, og = make()
    step = GraphedTrainStep(mg, og, _seq_loss, batches[0],
                            expected_entries=1 << 16,
                            expected_slots=1 << 16)
    assert step.graph is not None, "capture must succeed"
    assert mg.item_ev.graph_mode and mg.collection.graph_mode
    for b in batches[1:]:
        loss = step(b)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    mg.item_ev.storage._check_error()
    mg.collection.storage._check_error()

    # the eager twin trains on what the graph model really ran: the
    # example batch twice (warm-up), then the six replays
    me, oe = make()
    for b in [batches[0], batches[0]] + batches[1:]:
        le = _seq_loss(me, *b)
        oe.zero_grad()
        le.backward()
        oe.step()
    torch.cuda.synchronize()
    assert torch.isfinite(le)

    for eg, ee in ((mg.item_ev, me.item_ev), (mg.collection, me.collection)):
        kg, vg, fg, _ = (t.cpu() for t in eg.export())
        ke, ve, fe, _ = (t.cpu() for t in ee.export())
        ig, ie = torch.argsort(kg), torch.argsort(ke)
        assert torch.equal(kg[ig], ke[ie])
        assert torch.equal(fg[ig], fe[ie])
        # dense dW accumulates with fp32 atomics (order-nondeterministic):
        # eager and replay trajectories part at bf16 noise level, the
        # bound test_gpu_graph.py uses for the same reason
        torch.testing.assert_close(vg[ig], ve[ie], rtol=1e-2, atol=3e-3)
    assert not bool((mg.item_ev.export()[0] == 0).any())

    step.graph = None
    del step
    gc.collect()
    torch.cuda.synchronize()
