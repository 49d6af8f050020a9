"""Preconditions of tests/test_gpu_dense_fwd_pipeline.py, proven without a
GPU: at every shape of the forward K-loop cases the integer operands of
dense_reference.fwd_case survive bf16, every partial sum stays below 2**24
(operands in [-4, 4] and K <= 512 give at most 16 * 512 = 8192), and the
reference is exact in fp32 — so fp32 MFMA accumulation is exact in any
order and the GPU comparison may be bit-exact.
"""
import pytest
import torch

from tests import dense_reference as R

# (M, N, K), each the smallest shape that reaches its boundary of the
# forward kernel's K loop (full 32-wide steps, two register buffers, a
# prefetch of the next step, then the K tail)
PIPELINE_SHAPES = [
    (64, 64, 32),     # one full step: prologue is also the last step
    (64, 64, 64),     # two steps: both buffers, no loop iteration
    (64, 64, 96),     # three: one loop iteration, odd step count
    (64, 64, 160),    # five
    (64, 64, 16),     # tail only
    (64, 64, 40),     # one step + tail of 8
    (64, 64, 48),     # one step + tail of 16 (the benchmark's K = 368)
    (64, 64, 77),     # two steps + a K % 8 != 0 tail, unaligned rows
    (48, 64, 64),     # a wave past M
    (40, 64, 64),     # M % 16 != 0: clamped rows
    (80, 1, 64),      # N = 1
    (80, 17, 96),     # a partial second B tile
    (130, 136, 96),   # two full 64-column tiles through the LDS store
                      # path, a partial third, ragged M over blocks
    (128, 64, 512),   # the benchmark's 16 steps
]
NAN_SHAPE = (80, 72, 96)    # NaN containment at a multi-step K
ALL_SHAPES = PIPELINE_SHAPES + [NAN_SHAPE]


def test_shapes_cover_the_loop_boundaries():
    ks = {k for _, _, k in PIPELINE_SHAPES}
    assert {k // 32 for k in ks} >= {0, 1, 2, 3, 5, 16}
    assert {k % 32 for k in ks if k % 8 == 0} >= {0, 8, 16}
    assert any(k % 8 for k in ks)
    assert all(k <= 512 for _, _, k in ALL_SHAPES)
    assert len(set(ALL_SHAPES)) == len(ALL_SHAPES)


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
