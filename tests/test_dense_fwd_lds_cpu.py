"""Preconditions of tests/test_gpu_dense_fwd_lds.py, proven without a GPU:
at every shape of the LDS-staged forward kernel's cases the integer
operands of dense_reference.fwd_case survive bf16, every partial sum stays
below 2**24 (operands in [-4, 4] and K <= 512 give at most 16 * 512 = 8192)
and the reference is exact in fp32 — so fp32 MFMA accumulation is exact in
any order and the GPU comparison may be bit-exact.
"""
import pytest
import torch

from tests import dense_reference as R

CHUNK = 64   # K elements k_linear_fwd_lds stages per barrier
TILE = 64    # rows and columns of a block tile; a wave takes 16 rows

# (M, N, K), each the smallest shape that reaches its boundary of the
# kernel's chunk pipeline (two LDS buffers, one barrier per chunk)
LDS_SHAPES = [
    (64, 64, 64),     # one chunk
    (64, 64, 128),    # two chunks, both buffers
    (64, 64, 192),    # three chunks, the first buffer is reused
    (64, 64, 40),     # K shorter than a chunk
    (16, 64, 128),    # waves 1-3 entirely past M must still run the barriers
    (17, 64, 128),    # a wave with one live row
    (70, 72, 200),    # a second block in both directions with 6 and 8 live
                      # rows, clamped rows, a K tail of 8
    (128, 128, 368),  # the benchmark's 48-wide tail after five chunks
    (130, 136, 96),   # run with act 0 and no bias
    (64, 1, 128),     # N = 1
    (64, 64, 72),     # run with W at an odd bf16 element
]
NAN_SHAPE = (80, 72, 192)   # NaN containment, the NaN in the third chunk
FALLBACK_SHAPE = (64, 64, 77)   # K % 8 != 0: linear_fwd_lds refuses it
ALL_SHAPES = LDS_SHAPES + [NAN_SHAPE, FALLBACK_SHAPE]


def test_shapes_cover_the_pipeline_boundaries():
    ks = {k for _, _, k in LDS_SHAPES}
    assert {-(-k // CHUNK) for k in ks} >= {1, 2, 3, 4, 6}
    # tails: none, shorter than one 32-wide step, longer than one
    assert {k % CHUNK for k in ks} >= {0, 8, 40, 48}
    assert all(k % 8 == 0 for k in ks) and FALLBACK_SHAPE[2] % 8
    ms = {m for m, _, _ in LDS_SHAPES}
    assert any(m <= 16 for m in ms)                 # idle waves
    assert any(m % 16 == 1 for m in ms)             # one live row
    assert any(m > TILE and m % TILE for m in ms)   # ragged second block
    ns = {n for _, n, _ in LDS_SHAPES}
    assert 1 in ns and any(n > TILE and n % TILE for n in ns)
    assert all(k <= 512 for _, _, k in ALL_SHAPES)
    assert len(set(ALL_SHAPES)) == len(ALL_SHAPES)
    m, n, k = NAN_SHAPE
    assert k == 3 * CHUNK and m % TILE and n % TILE


@pytest.mark.parametrize("m,n,k", ALL_SHAPES)
def test_operands_survive_bf16(m, n, k):
    c = R.fwd_case(m, n, k)
    assert c["x"].shape == (m, k) and c["w"].shape == (n, k)
    assert R.bf16_exact(c["x"].double())
    assert R.bf16_exact(c["w"].double())
    assert R.bf16_exact(c["bias"])
    lo, hi = R.FWD_RANGE
    assert int(c["x"].min()) >= lo and int(c["x"].max()) <= hi
    assert int(c["w"].min()) >= lo and int(c["w"].max()) <= hi


@pytest.mark.parametrize("m,n,k", ALL_SHAPES)
def test_partial_sums_are_exact_in_fp32(m, n, k):
    c = R.fwd_case(m, n, k)
    peak = c["x"].abs() @ c["w"].abs().t()
    total = peak.double() + c["bias"].abs().double()
    assert float(total.max()) <= 16 * 512 + 2
    assert float(total.max()) < R.EXACT_LIMIT


@pytest.mark.parametrize("m,n,k", ALL_SHAPES)
def test_reference_is_exact_in_fp32(m, n, k):
    c = R.fwd_case(m, n, k)
    for pre in (c["pre_bias"], c["pre_nobias"]):
        assert torch.equal(pre.float().double(), pre)
        # to_bf16_rne asserts the same and rounds once
        assert R.to_bf16_rne(torch.relu(pre)).dtype == torch.bfloat16
