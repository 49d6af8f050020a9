"""The fused_cross_train flag off the GPU: same parameters, same outputs and
gradients, and cross_stack refuses a CPU tensor."""
import pytest
import torch

from deeprec_amd.models.zoo import DCN, MLPerfDLRMDCN, _CrossNet
from deeprec_amd.ops.fused_cross import cross_stack


@pytest.mark.parametrize("v2,low_rank", [(False, 0), (True, 0), (True, 5)])
def test_flag_changes_nothing_on_the_cpu(v2, low_rank):
    torch.manual_seed(0)
    plain = _CrossNet(45, 3, v2, low_rank)
    fused = _CrossNet(45, 3, v2, low_rank, fused_train=True)
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    x0 = torch.randn(33, 45)
    outs = [net(x0) for net in (plain, fused)]
    assert torch.equal(*outs)
    for out in outs:
        out.square().sum().backward()
    for p, q in zip(plain.parameters(), fused.parameters()):
        assert torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("cls", [MLPerfDLRMDCN, DCN])
def test_models_pass_the_flag_on(cls):
    plain, fused = cls(device="cpu"), cls(device="cpu", fused_cross_train=True)
    assert fused.cross.fused_train and not plain.cross.fused_train
    assert list(fused.state_dict()) == list(plain.state_dict())


def test_cross_stack_refuses_a_cpu_tensor():
    with pytest.raises(ValueError, match="GPU"):
        cross_stack(torch.zeros(4, 8), [(torch.zeros(8, 8), torch.zeros(8))])
