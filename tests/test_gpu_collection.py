"""GPU EmbeddingCollection: fused group kernels vs CPU reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from deeprec_amd import EmbeddingVariableOption, RaggedIds  # noqa: E402
from deeprec_amd.embedding.collection import EmbeddingCollection  # noqa: E402
from deeprec_amd.embedding.options import InitializerOption  # noqa: E402

DEV = "cuda:0"


def _pair(name, n_tables=4, dim=16, combiners=None):
    def init(t):
        gen = torch.Generator().manual_seed(7)
        t.normal_(0, 1, generator=gen)

    combiners = combiners or ["mean"] * n_tables
    names = [f"t{i}" for i in range(n_tables)]
    opt = EmbeddingVariableOption(
        init_option=InitializerOption(initializer=init, default_value_dim=8))
    cg = EmbeddingCollection(f"{name}_g", names, dim, ev_option=opt,
                             combiners=combiners, device=DEV)
    cc = EmbeddingCollection(f"{name}_c", names, dim, ev_option=opt,
                             combiners=combiners, device="cpu")
    torch.testing.assert_close(cg.storage.default_values.cpu(),
                               cc.storage.default_values)
    return cg, cc


def _rand_sp(batch, max_len, card, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, max_len + 1, (batch,), generator=g)
    vals = torch.randint(0, card, (int(lens.sum()),), generator=g)
    offs = torch.zeros(batch + 1, dtype=torch.int32)
    offs[1:] = lens.cumsum(0).to(torch.int32)
    return RaggedIds(vals, offs)


def test_group_forward_matches_cpu():
    cg, cc = _pair("fwd", combiners=["sum", "mean", "sqrtn", "mean"])
    sp = [_rand_sp(256, 6, 1000, 10 + t) for t in range(4)]
    out_g = cg.lookup([s.to(DEV) for s in sp])
    out_c = cc.lookup(sp)
    torch.testing.assert_close(out_g.cpu(), out_c, rtol=1e-5, atol=1e-5)


def test_group_weighted_matches_cpu():
    cg, cc = _pair("w", n_tables=2, combiners=["mean", "sqrtn"])
    sp = []
    for t in range(2):
        s = _rand_sp(64, 4, 100, 20 + t)
        s.weights = torch.rand(s.nnz) + 0.1
        sp.append(s)
    out_g = cg.lookup([s.to(DEV) for s in sp])
    out_c = cc.lookup(sp)
    torch.testing.assert_close(out_g.cpu(), out_c, rtol=1e-5, atol=1e-5)


def test_group_backward_and_training_matches_cpu():
    from deeprec_amd.optimizers import AdagradOptimizer
    cg, cc = _pair("train", n_tables=3, dim=8)
    og = AdagradOptimizer(embedding_variables=[cg], learning_rate=0.1)
    oc = AdagradOptimizer(embedding_variables=[cc], learning_rate=0.1)
    for step in range(3):
        sp = [_rand_sp(128, 4, 200, 100 * step + t) for t in range(3)]
        out_g = cg.lookup([s.to(DEV) for s in sp])
        out_c = cc.lookup(sp)
        (out_g ** 2).sum().backward()
        (out_c ** 2).sum().backward()
        og.step()
        oc.step()
    tg = cg.export_tables()
    tc = cc.export_tables()
    for name in tg:
        kg, vg, fg, _ = tg[name]
        kc, vc, fc, _ = tc[name]
        og_idx = torch.argsort(kg.cpu())
        oc_idx = torch.argsort(kc)
        torch.testing.assert_close(kg.cpu()[og_idx], kc[oc_idx])
        torch.testing.assert_close(vg.cpu()[og_idx], vc[oc_idx],
                                   rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(fg.cpu()[og_idx], fc[oc_idx])


def test_group_bf16_output():
    cg, _ = _pair("bf16", n_tables=2)
    sp = [_rand_sp(32, 3, 50, 5 + t).to(DEV) for t in range(2)]
    out = cg.lookup(sp, out_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.shape == (32, 32)
    ref = cg.lookup(sp, train=False)
    torch.testing.assert_close(out.float().cpu(), ref.cpu(), rtol=2e-2,
                               atol=2e-2)


def test_dlrm_collection_gpu_steps():
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.models.dlrm import DLRM
    from deeprec_amd.optimizers import AdamAsyncOptimizer
    torch.manual_seed(0)
    m = DLRM(device=DEV, bf16=True, use_collection=True)
    assert m.collection is not None
    ds = CriteoSyntheticDataset(batch_size=2048, device=DEV, seed=4)
    opt = AdamAsyncOptimizer(params=m.parameters(),
                             embedding_variables=m.embedding_variables())
    for i, (dense, sparse, labels) in enumerate(ds):
        if i >= 4:
            break
        loss = m.loss_fn(m(dense, sparse), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
    assert m.collection.size() > 0


def test_lookup_matrix_gpu_matches_cpu():
    cg, cc = _pair("mat", n_tables=5, dim=16)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 500, (512, 5), generator=g)
    out_g = cg.lookup_matrix(ids.to(DEV))
    out_c = cc.lookup_matrix(ids)
    torch.testing.assert_close(out_g.cpu(), out_c, rtol=1e-5, atol=1e-5)


def test_lookup_matrix_gpu_training_matches_cpu():
    from deeprec_amd.optimizers import AdamOptimizer
    cg, cc = _pair("mat_t", n_tables=3, dim=8)
    og = AdamOptimizer(embedding_variables=[cg])
    oc = AdamOptimizer(embedding_variables=[cc])
    for step in range(3):
        g = torch.Generator().manual_seed(30 + step)
        # heavy duplication exercises the chunked backward
        ids = torch.randint(0, 7, (1024, 3), generator=g)
        out_g = cg.lookup_matrix(ids.to(DEV))
        out_c = cc.lookup_matrix(ids)
        (out_g ** 2).sum().backward()
        (out_c ** 2).sum().backward()
        og.step()
        oc.step()
    tg, tc = cg.export_tables(), cc.export_tables()
    for name in tg:
        kg, vg, _, _ = tg[name]
        kc, vc, _, _ = tc[name]
        oi, ci = torch.argsort(kg.cpu()), torch.argsort(kc)
        torch.testing.assert_close(vg.cpu()[oi], vc[ci], rtol=1e-4,
                                   atol=1e-5)


@pytest.mark.gpu
def test_async_embedding_stage_gpu():
    """Side-stream pipelined lookups train correctly (1-step staleness
    allowed — assert convergence-compatible invariants, not equality)."""
    from deeprec_amd.embedding.collection import EmbeddingCollection
    from deeprec_amd.optimizers import AdamAsyncOptimizer
    from deeprec_amd.training.async_stage import AsyncEmbeddingStage

    torch.manual_seed(0)
    names = [f"t{i}" for i in range(4)]
    coll = EmbeddingCollection("async_gpu", names, 16, device="cuda")
    opt = AdamAsyncOptimizer(embedding_variables=[coll])
    stage = AsyncEmbeddingStage(coll)
    batches = [torch.randint(0, 500, (64, 4), device="cuda")
               for _ in range(8)]
    stage.submit(batches[0])
    for i in range(8):
        emb = stage.take()
        if i + 1 < len(batches):
            stage.submit(batches[i + 1])
        loss = (emb.float() ** 2).mean()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    coll.storage._check_error()
    assert torch.isfinite(loss)
    assert coll.size() > 0


def test_interleaved_lookups_keep_their_own_rank():
    """Two lookup_matrix forwards before either backward, the first on the
    hash-dedup path (pass C rank -> csr_scatter), the second on the sort
    path (no rank -> csr_order): each backward must scatter with the CSR
    of its own lookup. Integer grads make every sum exact in fp32, so the
    per-key gradients must EQUAL a CPU index_add_; keys are matched by
    value because atomics decide the dedup path's unique order."""
    batch, n_tables, dim = 64, 3, 16
    coll = EmbeddingCollection("rank", ["a", "b", "c"], dim, device=DEV)
    st = coll.storage
    gen = torch.Generator().manual_seed(31)

    def make(base):
        ids = torch.randint(base, base + 50, (batch, n_tables),
                            generator=gen)
        for t in range(n_tables):  # one hot id per table, ~20 occurrences
            rows = torch.randperm(batch, generator=gen)[:20]
            ids[rows, t] = base + 7 * t
        g = torch.randint(-4, 5, (batch, n_tables * dim), generator=gen)
        return ids, g.to(torch.bfloat16)

    (ids1, g1), (ids2, g2) = make(0), make(25)
    assert st.prefers_dedup()
    out1 = coll.lookup_matrix(ids1.to(DEV), out_dtype=torch.bfloat16)
    st._uniq_ratio = 0.99  # above the dedup threshold: sort path next
    assert not st.prefers_dedup()
    out2 = coll.lookup_matrix(ids2.to(DEV), out_dtype=torch.bfloat16)
    out1.backward(g1.to(DEV))
    out2.backward(g2.to(DEV))
    grads = coll.consume_grads()
    assert len(grads) == 2
    tags = (torch.arange(n_tables) << 48).repeat_interleave(batch)
    for (slots, keys, gu), ids, g in zip(grads, (ids1, ids2), (g1, g2)):
        occ_keys = ids.t().reshape(-1) + tags  # occurrence t * batch + b
        occ_grad = g.float().reshape(batch, n_tables, dim) \
            .permute(1, 0, 2).reshape(-1, dim)
        ref_keys, inv = torch.unique(occ_keys, return_inverse=True)
        ref = torch.zeros(ref_keys.numel(), dim).index_add_(0, inv, occ_grad)
        order = torch.argsort(keys.cpu())
        assert torch.equal(keys.cpu()[order], ref_keys)
        assert torch.equal(gu.cpu().float()[order], ref)
    st._check_error()
