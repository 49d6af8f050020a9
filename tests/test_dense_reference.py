"""Preconditions of the exact-integer linear-kernel references (CPU only).

tests/test_gpu_dense_shapes.py compares the MFMA kernels bit for bit with
int64 matmuls. That is only sound if the inputs are what they claim to be;
this file proves it for every shape of the grid without a GPU."""
import pytest
import torch

from tests import dense_reference as R

ALL_DW_SHAPES = R.DW_SHAPES + [s for s in R.DW_OUT_SHAPES
                               if s not in R.DW_SHAPES]


def _is_small_int(t, rng):
    return (t.dtype == torch.int64 and int(t.min()) >= rng[0]
            and int(t.max()) <= rng[1] and R.bf16_exact(t))


@pytest.mark.parametrize("m,n,k", R.FWD_SHAPES)
def test_fwd_inputs_exact(m, n, k):
    c = R.fwd_case(m, n, k)
    assert c["x"].shape == (m, k) and c["w"].shape == (n, k)
    assert _is_small_int(c["x"], R.FWD_RANGE)
    assert _is_small_int(c["w"], R.FWD_RANGE)
    # per-element random: a transposed or shifted read changes the result
    assert c["x"].unique().numel() == R.FWD_RANGE[1] - R.FWD_RANGE[0] + 1
    b = c["bias"]
    assert b.dtype == torch.float32 and torch.equal(b * 2, (b * 2).round())
    assert (b != 0).any()
    # every partial sum is bounded by |x| @ |w|^T + |b|
    worst = (c["x"].abs() @ c["w"].abs().t()).double() + b.abs().double()
    assert float(worst.max()) < R.EXACT_LIMIT
    for pre in (c["pre_bias"], c["pre_nobias"]):
        assert torch.equal(pre.float().double(), pre)
    assert torch.equal(c["pre_nobias"], (c["x"].double()
                                         @ c["w"].double().t()))


@pytest.mark.parametrize("m,n,k", R.FWD_SHAPES)
def test_fwd_sigmoid_scaling(m, n, k):
    """The act = 2 cases scale w by 2**-s: still exact in bf16, and the
    pre-activations stay inside [-8, 8] where sigmoid is far from 0/1."""
    c = R.fwd_case(m, n, k)
    s = R.sigmoid_shift(c["ref"], c["bias"])
    assert 0 <= s <= 10
    w = c["w"].double() * 2.0 ** -s
    assert R.bf16_exact(w)
    pre = c["ref"].double() * 2.0 ** -s
    assert torch.equal(pre, c["x"].double() @ w.t())
    assert torch.equal(pre.float().double(), pre)
    assert float((pre.abs() + c["bias"].abs().double()).max()) \
        <= R.SIGMOID_LIMIT
    if s:  # not over-scaled: the range is used
        assert float(pre.abs().max()) > R.SIGMOID_LIMIT / 4


def test_fwd_rounding_is_exercised():
    """At least one fwd case rounds >= 5 % of its outputs, exact ties
    (half-integers between 128 and 256) included."""
    frac = {s: R.inexact_fraction(R.fwd_case(*s)["pre_bias"])
            for s in R.FWD_SHAPES}
    assert max(frac.values()) >= 0.05, frac
    ties = {s: R.tie_count(R.fwd_case(*s)["pre_bias"])
            for s in R.FWD_SHAPES}
    assert max(ties.values()) >= 16, ties
    # ties to both an even and an odd lower neighbour: truncation and
    # round-half-up are each wrong on one kind
    pre = R.fwd_case(80, 72, 429)["pre_bias"].float()
    bits = pre.view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    odd = ((bits >> 16) & 1) == 1
    assert int((tie & odd).sum()) > 0 and int((tie & ~odd).sum()) > 0


@pytest.mark.parametrize("m,n,k", R.DX_SHAPES)
def test_dx_inputs_exact(m, n, k):
    c = R.dx_case(m, n, k)
    assert c["g"].shape == (m, n) and c["w"].shape == (n, k)
    assert _is_small_int(c["g"], R.DX_RANGE)
    assert _is_small_int(c["w"], R.DX_RANGE)
    worst = c["g"].abs() @ c["w"].abs()
    assert int(worst.max()) < R.EXACT_LIMIT
    assert c["ref"].shape == (m, k)


def test_dx_rounding_is_exercised():
    frac = {s: R.inexact_fraction(R.dx_case(*s)["ref"].double())
            for s in R.DX_SHAPES}
    assert max(frac.values()) >= 0.05, frac
    # both dX kernels see it, not only one of them
    assert frac[(80, 127, 72)] >= 0.05 and frac[(130, 300, 45)] >= 0.05, frac


@pytest.mark.parametrize("m,n,k", ALL_DW_SHAPES)
def test_dw_inputs_exact(m, n, k):
    c = R.dw_case(m, n, k)
    assert c["g"].shape == (m, n) and c["x"].shape == (m, k)
    assert _is_small_int(c["g"], R.DW_RANGE)
    assert _is_small_int(c["x"], R.DW_RANGE)
    worst = c["g"].abs().t() @ c["x"].abs()
    assert int(worst.max()) < R.EXACT_LIMIT
    assert int(c["g"].abs().sum(0).max()) < R.EXACT_LIMIT
    assert c["dw"].shape == (n, k) and c["db"].shape == (n,)
    # the results are fp32-exact, so torch.equal in fp32 is meaningful
    assert torch.equal(c["dw"].float().long(), c["dw"])
    assert torch.equal(c["db"].float().long(), c["db"])
    # the result is dense: a dropped tile or chunk cannot hide among zeros
    assert (c["dw"] != 0).any(1).all() and (c["db"] != 0).any()
    if n * k >= 45:
        assert (c["dw"] != 0).double().mean() > 0.9


def test_dw_multi_chunk_case_stays_multi_chunk():
    m_chunks, cpb = R.dw_cpb(4934, 200, 429)
    assert (m_chunks, cpb) == (39, 2)
    assert m_chunks % cpb != 0
    # the other shapes run one chunk per block
    for s in R.DW_SHAPES[:-1]:
        assert R.dw_cpb(*s)[1] == 1


def test_dw_out_sizes_have_a_tail():
    for m, n, k in R.DW_OUT_SHAPES:
        assert (n * k + n) % 4 != 0 and (n * k) % 4 != 0
    assert R.DW_OUT_SHAPES[0][1] < 64 <= R.DW_OUT_SHAPES[1][1]
    m, n, k = R.DW_OUT_SHAPES[2]
    assert n * k + n < 4


def test_carve_and_guard_check():
    v = torch.arange(12, dtype=torch.float32).view(3, 4)
    view, flat, off = R.carve(v, "cpu", offset=5, tail=7)
    assert view.is_contiguous() and torch.equal(view, v)
    assert view.data_ptr() == flat.data_ptr() + 5 * 4
    assert flat.numel() == 5 + 12 + 7
    assert R.outside_untouched(flat, off, 12, float("nan"))
    flat[3] = 0.0
    assert not R.outside_untouched(flat, off, 12, float("nan"))
    view, flat, off = R.carve(v, "cpu", offset=3, tail=2, fill=-7.0)
    assert R.outside_untouched(flat, off, 12, -7.0)
    flat[-1] = 0.0
    assert not R.outside_untouched(flat, off, 12, -7.0)


def test_to_bf16_rne_rounds_ties_to_even():
    x = torch.tensor([128.5, 129.5, 257.0, 259.0, -130.5, 3.0],
                     dtype=torch.float64)
    want = torch.tensor([128.0, 130.0, 256.0, 260.0, -130.0, 3.0])
    assert torch.equal(R.to_bf16_rne(x).float(), want)
    assert R.tie_count(x) == 5
    assert abs(R.inexact_fraction(x) - 5 / 6) < 1e-12
    with pytest.raises(AssertionError):
        R.to_bf16_rne(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))


def test_linear_bounds():
    a = torch.tensor([[1.0, -2.0]], dtype=torch.float64)
    b = torch.tensor([[3.0], [4.0]], dtype=torch.float64)
    full, acc = R.linear_bounds(a, b, a @ b, 2)
    assert float(acc) == 2 * 2.0 ** -23 * 11.0
    assert float(full) == 2.0 ** -8 * 5.0 + float(acc)
