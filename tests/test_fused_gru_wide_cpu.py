"""FusedGRU, DIEN and the runner at recurrent widths above 32 (CPU).

The reference DIEN runs a 36-wide item embedding and HIDDEN_SIZE = 36;
FusedGRU takes hidden sizes up to 64 (the tile kernels' limit on the GPU,
tests/test_gpu_gru_tile.py; the CPU path is the plain reference loop)."""
import pytest
import torch

from deeprec_amd.ops.fused_gru import FusedGRU


@pytest.mark.parametrize("hidden", [36, 64])
def test_fused_gru_wide_matches_torch_gru_and_trains(hidden):
    torch.manual_seed(0)
    gru = FusedGRU(20, hidden)
    assert gru.weight_hh_l0.shape == (3 * hidden, hidden)
    x = torch.randn(4, 6, 20, requires_grad=True)
    alpha = torch.rand(4, 6, requires_grad=True)
    out = gru(x, alpha)
    assert out.shape == (4, 6, hidden)
    out.sum().backward()
    for name, t in [("x", x), ("alpha", alpha)] + list(gru.named_parameters()):
        assert t.grad is not None and torch.isfinite(t.grad).all(), name
        assert float(t.grad.abs().max()) > 0, name
    assert len(list(gru.parameters())) == 4
    # matches torch GRU when alpha is None and weights are shared
    ref = torch.nn.GRU(20, hidden, batch_first=True)
    with torch.no_grad():
        ref.weight_ih_l0.copy_(gru.weight_ih_l0)
        ref.weight_hh_l0.copy_(gru.weight_hh_l0)
        ref.bias_ih_l0.copy_(gru.bias_ih_l0)
        ref.bias_hh_l0.copy_(gru.bias_hh_l0)
    out2 = gru(x.detach(), None)
    out_ref, _ = ref(x.detach())
    torch.testing.assert_close(out2, out_ref, rtol=1e-4, atol=1e-5)


def test_fused_gru_hidden_limit_and_impl():
    with pytest.raises(AssertionError, match="64"):
        FusedGRU(8, 65)
    assert FusedGRU(8, 64).tile and FusedGRU(8, 33).tile
    # auto keeps the wave kernels wherever they reach
    assert not FusedGRU(8, 32).tile and not FusedGRU(8, 1).tile
    assert FusedGRU(8, 32, impl="tile").tile
    assert not FusedGRU(8, 32, impl="wave").tile
    with pytest.raises(ValueError, match="32"):
        FusedGRU(8, 33, impl="wave")
    with pytest.raises(AssertionError):
        FusedGRU(8, 16, impl="mfma")


def test_reference_dien_widths_train():
    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.models.sequence import DIEN
    from deeprec_amd.optimizers import AdagradOptimizer
    torch.manual_seed(0)
    m = DIEN(item_dim=36, gru_hidden=36, device="cpu", bf16=False)
    assert m.gru.hidden_size == 36 and m.gru.input_size == 36
    assert m.augru.hidden_size == 36 and m.augru.input_size == 36
    ds = CriteoSyntheticDataset(batch_size=16, seed=4)
    opt = AdagradOptimizer(params=m.parameters(),
                           embedding_variables=m.embedding_variables(),
                           learning_rate=0.01)
    for i in range(2):
        dense, ids, seq, target, labels = ds.next_seq_batch(seq_len=20)
        out = m(dense, ids[:, :m.num_sparse], seq, target)
        loss = m.loss_fn(out, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
    assert m.item_ev.size() > 0


def test_runner_width_flags():
    from deeprec_amd.models.runner import build_argparser, width_kwargs
    p = build_argparser()
    args = p.parse_args(["--model", "dien", "--gru_hidden", "36",
                         "--item_dim", "36"])
    assert args.gru_hidden == 36 and args.item_dim == 36
    assert width_kwargs(args) == {"gru_hidden": 36, "item_dim": 36}
    # not given: the model's own defaults, nothing passed
    args = p.parse_args(["--model", "dien"])
    assert args.gru_hidden is None and args.item_dim is None
    assert width_kwargs(args) == {}
    assert width_kwargs(p.parse_args(["--model", "din", "--item_dim",
                                      "36"])) == {"item_dim": 36}
    # a model that takes neither
    assert width_kwargs(p.parse_args(["--model", "dlrm"])) == {}
    with pytest.raises(SystemExit):
        width_kwargs(p.parse_args(["--model", "din", "--gru_hidden", "36"]))
