"""The fused_cross flag off the GPU: same parameters, same results, and the
models that carry it still train."""
import pytest
import torch

from deeprec_amd.data.synthetic import CriteoSyntheticDataset
from deeprec_amd.models.zoo import DCN, _CrossNet
from deeprec_amd.optimizers import AdagradOptimizer


@pytest.mark.parametrize("v2,low_rank", [(False, 0), (True, 0), (True, 5)])
def test_fused_flag_changes_nothing_on_the_cpu(v2, low_rank):
    torch.manual_seed(0)
    plain = _CrossNet(45, 3, v2, low_rank)
    fused = _CrossNet(45, 3, v2, low_rank, fused=True)
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    plain.load_state_dict(fused.state_dict())
    x0 = torch.randn(33, 45)
    assert torch.equal(fused(x0), plain(x0))


def test_dcnv2_with_fused_cross_trains_on_the_cpu():
    torch.manual_seed(0)
    m = DCN(v2=True, fused_cross=True, device="cpu", bf16=False)
    assert m.cross.fused
    ds = CriteoSyntheticDataset(batch_size=32, seed=3, matrix_format=True)
    opt = AdagradOptimizer(params=m.parameters(),
                           embedding_variables=m.embedding_variables(),
                           learning_rate=0.01)
    dense, ids, labels = ds.next_batch()
    loss = m.loss_fn(m(dense, ids), labels)
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    assert all(p.grad is not None for p in m.cross.parameters())
