"""FusedMLP off the GPU: still an nn.Sequential in every way that callers
and checkpoints see, and numerically the plain per-layer torch path."""
from collections import OrderedDict

import torch
import torch.nn as nn

from deeprec_amd.ops.fused_mlp import FusedLinear, FusedMLP, fused_mlp


def _mlp():
    torch.manual_seed(4)
    return fused_mlp([24, 8, 1], 13, final_activation=False)


def test_state_dict_keys_and_container_behaviour():
    mlp = _mlp()
    assert isinstance(mlp, FusedMLP) and isinstance(mlp, nn.Sequential)
    assert list(mlp.state_dict().keys()) == [
        "0.weight", "0.bias", "1.weight", "1.bias", "2.weight", "2.bias"]
    assert len(mlp) == 3 and isinstance(mlp[0], FusedLinear)
    assert [m.out_features for m in mlp] == [24, 8, 1]
    assert [m.activation for m in mlp] == ["relu", "relu", None]
    assert sum(isinstance(m, FusedLinear) for m in mlp.modules()) == 3
    # a plain Sequential of the same layers loads the same checkpoint
    plain = nn.Sequential(*[FusedLinear(m.in_features, m.out_features)
                            for m in mlp])
    plain.load_state_dict(mlp.state_dict())
    assert torch.equal(plain[2].weight, mlp[2].weight)


def test_slicing_and_ordered_dict_construction():
    mlp = _mlp()
    head = mlp[:2]
    assert isinstance(head, FusedMLP) and len(head) == 2
    assert head[0] is mlp[0] and head[1] is mlp[1]
    assert list(head.state_dict().keys()) == [
        "0.weight", "0.bias", "1.weight", "1.bias"]
    named = FusedMLP(OrderedDict([("a", mlp[0]), ("b", mlp[1])]))
    assert list(named.state_dict().keys()) == [
        "a.weight", "a.bias", "b.weight", "b.bias"]
    x = torch.randn(5, 13)
    assert torch.equal(named(x), head(x))
    assert torch.equal(mlp[2](head(x)), mlp(x))


def test_cpu_forward_backward_equal_plain_sequential():
    mlp = _mlp()
    plain = nn.Sequential(*list(mlp))      # the same layer objects
    x = torch.randn(37, 13)
    go = torch.randn(37, 1)

    def run(model):
        for p in model.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        out = model(xi)
        out.backward(go)
        return [out.detach(), xi.grad] + [p.grad.clone()
                                          for p in model.parameters()]

    for a, b in zip(run(mlp), run(plain)):
        assert torch.equal(a, b)
    # and the layers compute what torch's own Linear + ReLU compute
    ref = x
    for m in mlp:
        ref = nn.functional.linear(ref, m.weight, m.bias)
        if m.activation == "relu":
            ref = torch.relu(ref)
    assert torch.equal(mlp(x), ref)
    # 3-D input: leading dimensions are kept
    assert mlp(torch.randn(2, 16, 13)).shape == (2, 16, 1)
