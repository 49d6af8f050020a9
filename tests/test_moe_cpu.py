"""The fused_experts flag and expert_mixture off the GPU: same parameters,
the same results as the per-expert path, and limits met by falling back."""
import pytest
import torch

from deeprec_amd.models.zoo import MMoE, PLE
from deeprec_amd.ops.fused_moe import MAX_EXPERTS, expert_mixture


@pytest.mark.parametrize("cls", [MMoE, PLE])
def test_fused_flag_changes_nothing_on_the_cpu(cls):
    kw = dict(embedding_dim=4, expert_sizes=(32, 16), device="cpu",
              bf16=False)
    torch.manual_seed(0)
    plain, fused = cls(**kw), cls(fused_experts=True, **kw)
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    emb = torch.randn(33, 26, 4)
    for m in (plain, fused):
        m.sparse_feats = lambda ids, train=True: emb
    dense = torch.randn(33, 13)
    for a, b in zip(fused(dense, None), plain(dense, None)):
        assert torch.equal(a, b)


def test_more_experts_than_the_kernels_take_fall_back():
    torch.manual_seed(0)
    n = MAX_EXPERTS + 1
    experts = [torch.nn.Linear(5, 3) for _ in range(n)]
    x, gate = torch.randn(16, 5), torch.randn(16, 2, n)
    mask = torch.ones(2, n, dtype=torch.uint8)
    mask[1, ::2] = 0
    out = expert_mixture(x, experts, gate, mask)
    ex = torch.stack([e(x) for e in experts], 1)
    for t in range(2):
        logit = gate[:, t].masked_fill(mask[t] == 0, float("-inf"))
        want = torch.einsum("be,beh->bh", torch.softmax(logit, 1), ex)
        torch.testing.assert_close(out[t], want)
    with pytest.raises(ValueError, match="mixes no expert"):
        expert_mixture(x, experts, gate, torch.zeros(2, n))
