"""The forward linear kernel's K loop at each of its boundaries.

k_linear_fwd_t loads a whole 32-wide K step at once from clamped
addresses, keeps the next step's loads in flight in a second register
buffer, zeroes rows past M / N with a select and handles the K tail as one
more step. The shapes (tests/test_dense_fwd_pipeline_cpu.py, which also
proves the exactness preconditions) reach: one, two, three and five full
steps, a tail alone, tails of 8 and 16, a K % 8 != 0 tail, a wave past M,
clamped rows, N = 1, partial B tiles, the LDS store path and the
benchmark's 16 steps. Integer-valued operands inside NaN guard bands,
bit-exact comparison, as in tests/test_gpu_dense_shapes.py.
"""
import pytest
import torch

from tests import dense_reference as R
from tests.test_dense_fwd_pipeline_cpu import NAN_SHAPE, PIPELINE_SHAPES
from tests.test_gpu_dense_shapes import (BF16, DEV, _assert_within,
                                         _bf16_operand, _check_fwd, _ext)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", [-1, 1])
@pytest.mark.parametrize("m,n,k", PIPELINE_SHAPES)
def test_fwd_pipeline_exact(m, n, k, variant):
    _check_fwd(m, n, k, variant, 1, True)


@pytest.mark.parametrize("variant", [-1, 1])
def test_fwd_pipeline_exact_plain(variant):
    """act 0 without bias: negative results reach the store unclipped."""
    _check_fwd(130, 136, 96, variant, 0, False)


@pytest.mark.parametrize("variant", [-1, 1])
def test_fwd_pipeline_weight_at_odd_element(variant):
    """Unaligned 16-byte loads in the main loop and in the tail of 8."""
    _check_fwd(64, 64, 40, variant, 1, True, w_offset=R.GUARD + 1)


@pytest.mark.parametrize("variant", [-1, 1])
def test_fwd_pipeline_nan_stays_in_its_row(variant):
    """One quiet NaN in the third K step of x, in a row whose block also
    holds clamped rows: exactly that output row is NaN, every other row is
    bit-identical to the clean run."""
    m, n, k = NAN_SHAPE
    row, col = 37, 70
    c = R.fwd_case(m, n, k)
    x = _bf16_operand(c["x"])
    w = _bf16_operand(c["w"])
    bias = R.carve(c["bias"], DEV)[0]
    clean = _ext().linear_fwd(x, w, bias, 1, variant).cpu()
    assert not torch.isnan(clean.float()).any()
    x[row, col] = torch.nan
    dirty = _ext().linear_fwd(x, w, bias, 1, variant).cpu()
    nan = torch.isnan(dirty.float())
    assert nan[row].all(), "the NaN did not reach every column"
    keep = torch.arange(m) != row
    assert not nan[keep].any(), "the NaN leaked into another row"
    assert torch.equal(dirty[keep].view(torch.int16),
                       clean[keep].view(torch.int16))


@pytest.mark.parametrize("variant", [-1, 1])
def test_fwd_pipeline_realistic_values(variant):
    """randn values on the bf16 grid at the benchmark's K, against fp64:
        |out - ref| <= 2**-8 |ref| + K 2**-23 (|x| @ |w|^T + |b|)
    — one bf16 rounding of the result plus fp32 accumulation over K terms,
    the bound test_fused_tower_against_fp64 derives."""
    m, n, k = 128, 64, 512
    gen = torch.Generator().manual_seed(29)
    x = torch.randn(m, k, generator=gen).to(BF16)
    w = torch.randn(n, k, generator=gen).to(BF16)
    b = torch.randn(n, generator=gen)
    out = _ext().linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1, variant)
    X, W, B = x.double(), w.double(), b.double()
    ref = torch.relu(X @ W.t() + B)
    bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * (X.abs() @ W.abs().t()
                                                      + B.abs())
    _assert_within(out, ref, bound, f"fwd {m}x{n}x{k} variant={variant}")
    assert (ref > 0).double().mean() > 0.2
