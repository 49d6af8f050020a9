"""dW (variant 2) and LDS dX with row-major LDS tiles and transposed reads.

Both kernels stage their tiles as they arrive (one 16-byte LDS store per
16-byte global load) and build each MFMA fragment from two transposed
reads of a 4-row x 16-column block. The shapes here are the smallest at
which that staging can go wrong: a chunk whose last 4-row block is only
partly real rows, padded columns inside a 16-column block, a ragged chunk
that follows a full one inside one block (a row of the previous chunk left
in LDS would be summed twice), idle waves that still have to stage, and a
K tail narrower than one column group.

Operands and references come from tests/dense_reference.py: integer-valued
bf16 matrices inside NaN-filled buffers, so fp32 accumulation is exact in
any order and every comparison is bit for bit.
"""
import functools

import pytest
import torch

from tests import dense_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16

DW_SHAPES = [
    (133, 64, 64),     # a full tile, then a second chunk of 5 rows
    (40, 65, 67),      # one short chunk, M % 8 != 0, N and K one column
                       # past a tile, odd K (unaligned global rows)
    (3996, 512, 368),  # cpb = 3, 11 chunk blocks, the last with 2 chunks,
                       # final chunk 28 rows
]
DX_SHAPES = [
    (36, 130, 4),      # one superchunk of 130 rows, K = 4, wave 1 with 4
                       # rows, waves 2-3 idle but staging
    (200, 515, 67),    # two full superchunks and a 3-row one, 3-column K
                       # tail, partly filled second M block
]


def _ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


def _bf16_operand(values):
    """Exact values -> bf16 view inside a NaN-filled device buffer."""
    v16 = values.double().to(BF16)
    assert torch.equal(v16.double(), values.double())
    return R.carve(v16, DEV)[0]


def _assert_bits_equal(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{what}: {got.dtype}{tuple(got.shape)} vs " \
        f"{want.dtype}{tuple(want.shape)}"
    assert not torch.isnan(got.float()).any(), \
        f"{what}: NaN in the output — a guard band was read and used"
    idt = torch.int16 if got.dtype == BF16 else torch.int32
    bad = got.view(idt) != want.view(idt)
    if bad.any():
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; "
            f"first at {i}: got {got[i].item()}, want {want[i].item()}; "
            f"rows {idx[:, 0].unique().tolist()[:12]}, "
            f"cols {idx[:, -1].unique().tolist()[:12]}")


@functools.lru_cache(maxsize=None)
def _dw_case(m, n, k):
    """R.dw_case; for the large shape the same operands with an fp64
    matmul, exact at these magnitudes (|sum| <= 9 m < 2**53) and much
    faster than int64 on the CPU."""
    if m * n * k < 10 ** 8:
        return R.dw_case(m, n, k)
    seed = 3000017 * m + 3001 * n + k
    g = R.int_matrix(m, n, R.DW_RANGE, seed)
    x = R.int_matrix(m, k, R.DW_RANGE, seed + 1)
    dw = (g.double().t() @ x.double())
    assert float(dw.abs().max()) < R.EXACT_LIMIT
    return {"g": g, "x": x, "dw": dw.long(), "db": g.sum(0)}


@pytest.mark.parametrize("want_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("m,n,k", DW_SHAPES)
def test_dw_variant2_exact(m, n, k, want_bias):
    if (m, n, k) == DW_SHAPES[-1]:
        # the only case with a ragged chunk behind full ones in one block;
        # a change of the cpb heuristic must not silently empty it
        m_chunks, cpb = R.dw_cpb(m, n, k)
        assert (m_chunks, cpb) == (32, 3) and m % 128 == 28
    c = _dw_case(m, n, k)
    g = _bf16_operand(c["g"])
    x = _bf16_operand(c["x"])
    dw, db = _ext().linear_dw(g, x, want_bias, 2)
    assert dw.shape == (n, k) and dw.dtype == torch.float32
    what = f"dW {m}x{n}x{k} variant=2"
    _assert_bits_equal(dw, c["dw"].float(), what + " dW")
    if want_bias:
        _assert_bits_equal(db, c["db"].float(), what + " dbias")
    else:
        assert db is None or db.numel() == 0


@pytest.mark.parametrize("m,n,k", DX_SHAPES)
def test_dx_lds_exact(m, n, k):
    assert n >= 128, "below the dispatch threshold of the LDS kernel"
    c = R.dx_case(m, n, k)
    g = _bf16_operand(c["g"])
    w = _bf16_operand(c["w"])
    dx = _ext().linear_dx(g, w)
    assert dx.shape == (m, k) and dx.dtype == BF16
    _assert_bits_equal(dx, R.to_bf16_rne(c["ref"].double()),
                       f"dX {m}x{n}x{k}")


@pytest.mark.parametrize("m,n,k", DX_SHAPES)
def test_dx_lds_epilogue_equals_dx_then_act_bwd(m, n, k):
    ext = _ext()
    c = R.dx_case(m, n, k)
    g = _bf16_operand(c["g"])
    w = _bf16_operand(c["w"])
    gen = torch.Generator().manual_seed(7 * m + k)
    prev = (torch.randint(-4, 9, (m, k), generator=gen).float() / 8).to(BF16)
    prev[0, 0] = 0.0
    prev[m - 1, k - 1] = -0.0
    prev_d = R.carve(prev, DEV)[0]
    want = ext.act_bwd(ext.linear_dx(g, w), prev_d, 1).cpu()
    got = ext.linear_dx(g, w, prev_d, 1)
    _assert_bits_equal(got, want, f"dX+relu {m}x{n}x{k}")
    dx = R.to_bf16_rne(c["ref"].double())
    _assert_bits_equal(
        got, torch.where(prev.float() > 0, dx, torch.zeros_like(dx)),
        f"dX+relu {m}x{n}x{k} vs int64")
