"""The LDS-staged forward linear kernel at each boundary of its pipeline.

k_linear_fwd_lds stages A[64][64] and W[64][64] per 64-wide K chunk into
one of two swizzled LDS buffers with one barrier per chunk, zero-fills rows
past M / N and 16-byte pieces past K with a select before the LDS store,
and shares tile shape, MFMA order and epilogue with k_linear_fwd_t<1>. The
shapes (tests/test_dense_fwd_lds_cpu.py, which also proves the exactness
preconditions) reach: one, two and three chunks, K shorter than a chunk,
waves wholly past M (which must still run the barriers), a wave with one
live row, ragged second blocks, K tails of 8 and 48, N = 1 and W at an odd
element. Every case runs through the linear_fwd_lds binding and through
linear_fwd(..., -1), which picks the kernel by shape. Integer-valued
operands inside NaN guard bands, bit-exact comparison, as in
tests/test_gpu_dense_shapes.py.
"""
import pytest
import torch

from tests import dense_reference as R
from tests.test_dense_fwd_lds_cpu import (FALLBACK_SHAPE, LDS_SHAPES,
                                          NAN_SHAPE)
from tests.test_gpu_dense_shapes import (BF16, DEV, _assert_bits_equal,
                                         _assert_within, _bf16_operand,
                                         _check_fwd, _ext)

pytestmark = pytest.mark.gpu

PLAIN_SHAPE = (130, 136, 96)   # run with act 0 and no bias
ODD_W_SHAPE = (64, 64, 72)     # run with W at an odd element
ROUTES = ["lds", "auto"]


def _run(route, x, w, bias, act):
    if route == "lds":
        return _ext().linear_fwd_lds(x, w, bias, act)
    return _ext().linear_fwd(x, w, bias, act, -1)


def _check(route, m, n, k, act, with_bias, w_offset=R.GUARD):
    if route == "auto":
        _check_fwd(m, n, k, -1, act, with_bias, w_offset=w_offset)
        return
    c = R.fwd_case(m, n, k)
    x = _bf16_operand(c["x"])
    w = _bf16_operand(c["w"], offset=w_offset)
    if with_bias:
        bias = R.carve(c["bias"], DEV)[0]
        pre = c["pre_bias"]
    else:
        bias = torch.empty(0, device=DEV)
        pre = c["pre_nobias"]
    out = _ext().linear_fwd_lds(x, w, bias, act)
    assert out.shape == (m, n) and out.dtype == BF16
    _assert_bits_equal(out, R.to_bf16_rne(R.apply_act(pre, act)),
                       f"fwd_lds {m}x{n}x{k} act={act} bias={with_bias}")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize(
    "m,n,k", [s for s in LDS_SHAPES if s not in (PLAIN_SHAPE, ODD_W_SHAPE)])
def test_fwd_lds_exact(m, n, k, route):
    _check(route, m, n, k, 1, True)


@pytest.mark.parametrize("route", ROUTES)
def test_fwd_lds_exact_plain(route):
    """act 0 without bias: negative results reach the store unclipped."""
    _check(route, *PLAIN_SHAPE, 0, False)


@pytest.mark.parametrize("route", ROUTES)
def test_fwd_lds_weight_at_odd_element(route):
    """Unaligned 16-byte loads in the main chunk and in the tail."""
    _check(route, *ODD_W_SHAPE, 1, True, w_offset=R.GUARD + 1)


@pytest.mark.parametrize("route", ROUTES)
def test_fwd_lds_nan_stays_in_its_row(route):
    """One quiet NaN in the third chunk of x, in a block that also holds
    clamped rows: exactly that output row is NaN, every other row is
    bit-identical to the clean run."""
    m, n, k = NAN_SHAPE
    row, col = 37, 150
    c = R.fwd_case(m, n, k)
    x = _bf16_operand(c["x"])
    w = _bf16_operand(c["w"])
    bias = R.carve(c["bias"], DEV)[0]
    clean = _run(route, x, w, bias, 1).cpu()
    assert not torch.isnan(clean.float()).any()
    x[row, col] = torch.nan
    dirty = _run(route, x, w, bias, 1).cpu()
    nan = torch.isnan(dirty.float())
    assert nan[row].all(), "the NaN did not reach every column"
    keep = torch.arange(m) != row
    assert not nan[keep].any(), "the NaN leaked into another row"
    assert torch.equal(dirty[keep].view(torch.int16),
                       clean[keep].view(torch.int16))


def test_fwd_lds_bit_identical_to_the_direct_kernel():
    """randn values on the bf16 grid at the benchmark's K, with bias and
    ReLU: the same MFMAs in the same order as k_linear_fwd_t<1>, so the
    same bits; and against fp64
        |out - ref| <= 2**-8 |ref| + K 2**-23 (|x| @ |w|^T + |b|)
    — one bf16 rounding of the result plus fp32 accumulation over K terms,
    the bound tests/test_gpu_dense_fwd_pipeline.py derives."""
    m, n, k = 128, 128, 512
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(m, k, generator=gen).to(BF16)
    w = torch.randn(n, k, generator=gen).to(BF16)
    b = torch.randn(n, generator=gen)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    out = _ext().linear_fwd_lds(xd, wd, bd, 1)
    direct = _ext().linear_fwd(xd, wd, bd, 1, 0)
    assert torch.equal(out.view(torch.int16), direct.view(torch.int16))
    X, W, B = x.double(), w.double(), b.double()
    ref = torch.relu(X @ W.t() + B)
    bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * (X.abs() @ W.abs().t()
                                                      + B.abs())
    _assert_within(out, ref, bound, f"fwd_lds {m}x{n}x{k}")
    assert (ref > 0).double().mean() > 0.2


def test_fwd_lds_refuses_k_not_multiple_of_8_and_auto_falls_back():
    m, n, k = FALLBACK_SHAPE
    c = R.fwd_case(m, n, k)
    x = _bf16_operand(c["x"])
    w = _bf16_operand(c["w"])
    bias = R.carve(c["bias"], DEV)[0]
    with pytest.raises(RuntimeError, match=r"K = 77"):
        _ext().linear_fwd_lds(x, w, bias, 1)
    _check_fwd(m, n, k, -1, 1, True)
