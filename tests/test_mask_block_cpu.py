"""The fused_blocks flag and mask_block off the GPU: same parameters and
bit-identical results to the plain path."""
import torch

from deeprec_amd.models.zoo import MaskNet
from deeprec_amd.ops.fused_mask import mask_block


def test_fused_flag_changes_nothing_on_the_cpu():
    kw = dict(embedding_dim=4, hidden=32, n_blocks=2, device="cpu",
              bf16=False)
    torch.manual_seed(0)
    plain = MaskNet(**kw)
    torch.manual_seed(0)
    fused = MaskNet(fused_blocks=True, **kw)
    assert list(fused.state_dict()) == list(plain.state_dict())
    emb, dense = torch.randn(33, 26, 4), torch.randn(33, 13)
    grads = []
    for m in (plain, fused):
        m.sparse_feats = lambda ids, train=True: emb
        logits = m(dense, None)
        logits.square().sum().backward()
        grads.append([logits.detach()] + [q.grad for q in m.parameters()])
    assert len(grads[0]) == len(grads[1]) > 1
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_mask_block_on_cpu_is_the_torch_formula():
    torch.manual_seed(1)
    linear, norm = torch.nn.Linear(45, 24), torch.nn.LayerNorm(24)
    h, mask = torch.randn(7, 45), torch.randn(7, 45)
    want = torch.relu(torch.nn.functional.layer_norm(
        torch.nn.functional.linear(mask * h, linear.weight, linear.bias),
        (24,), norm.weight, norm.bias, norm.eps))
    assert torch.equal(mask_block(h, mask, linear, norm), want)
    # another input dtype: the parameters follow it
    got = mask_block(h.double(), mask.double(), linear, norm)
    assert got.dtype == torch.float64
    torch.testing.assert_close(got.float(), want)
