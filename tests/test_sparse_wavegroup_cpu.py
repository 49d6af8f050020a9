"""Preconditions of tests/test_gpu_sparse_wavegroup.py, proven without a
GPU: the backward inputs are exact in fp32 in any order of addition, and
each structural situation a case is named for really occurs in its input,
computed from the counts alone. This keeps the GPU cases from passing
vacuously.
"""
import pytest
import torch

from tests import wavegroup_reference as W

R = 8  # the committed group size; the GPU test asserts BWD_SEG_R == 8
DIMS = (8, 16, 24, 32)


def _struct(name, r, dim):
    span = W.span_of(r, dim)
    return W.structure(W.patterns(r, span)[name], r, span)


@pytest.mark.parametrize("dim", [8, 16])
def test_block_run_is_one_block_slice(dim):
    s = _struct("block_run", R, dim)
    assert s["run_is_a_block"] == 1
    # it touches no neighbouring block, yet group 0's head has nothing
    # before it in the block and the last group's run ends with the block
    assert s["cut_by_block_edge"] == 0 and s["cut_by_group_edge"] == 1
    assert s["single_partial_groups"] == W.BLOCK // W.lanes(dim) - 2


@pytest.mark.parametrize("dim", [8, 16])
def test_long_run_is_cut_by_block_edges(dim):
    span = W.span_of(R, dim)
    counts = W.patterns(R, span)["long_run_at_5"]
    (b, e), = [x for x in W.runs_of(counts) if x[1] - x[0] > 1]
    assert b == 5 and (e - 1) // span - b // span == 2   # three blocks
    s = W.structure(counts, R, span)
    assert s["cut_by_block_edge"] == 1
    assert s["single_partial_groups"] >= 2 * (span // R)


@pytest.mark.parametrize("dim", [8, 16])
def test_runs_of_r_plus_1_cut_most_group_edges(dim):
    span = W.span_of(R, dim)
    counts = W.patterns(R, span)["runs_of_r_plus_1"]
    s = W.structure(counts, R, span)
    n_edges = (s["nnz"] - 1) // R
    # an edge at 8k is a run boundary only where 9 divides k
    assert s["cut_by_group_edge"] >= n_edges - n_edges // (R + 1) - 1
    assert s["blocks"] >= 2 and s["cut_by_block_edge"] >= 1
    assert s["merged_to_plain_store"] >= span // R // 2
    assert s["blocks_without_cut"] == 0


@pytest.mark.parametrize("dim", [8, 16])
def test_two_runs_meet_in_one_group(dim):
    s = _struct("two_runs_meet", R, dim)
    assert s["blocks"] == 1 and s["head_and_tail_groups"] == 1
    assert s["cut_by_group_edge"] == 2 and s["merged_to_plain_store"] == 2


@pytest.mark.parametrize("dim", [8, 16])
def test_group_inside_run(dim):
    s = _struct("group_inside_run", R, dim)
    assert s["single_partial_groups"] == 2 and s["blocks"] == 1
    assert s["merged_to_plain_store"] == 1


@pytest.mark.parametrize("dim", [8, 16])
def test_all_ones_has_no_cut(dim):
    s = _struct("all_ones", R, dim)
    assert s["max_count"] == 1 and s["blocks"] == 3
    assert s["blocks_without_cut"] == s["blocks"]


def test_sizes():
    for n in W.SIZES:
        counts = W.patterns(R, W.span_of(R, 16))[f"nnz{n}"]
        assert sum(counts) == n and min(counts) >= 1
    s = _struct("nnz1031", R, 16)
    assert s["blocks"] == 9 and s["cut_by_block_edge"] >= 1
    assert s["nnz"] % R != 0            # groups past nnz in the last block
    assert _struct("nnz7", R, 16)["cut_by_group_edge"] == 0
    assert _struct("nnz129", R, 16)["blocks"] == 2


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("r", W.R_SWEEP)
def test_mixed_holds_every_situation(r, dim):
    """The pattern of the shape, type and R sweeps."""
    s = _struct("mixed", r, dim)
    assert s["cut_by_block_edge"] >= 1
    assert s["merged_to_plain_store"] >= 1
    assert s["single_partial_groups"] >= 1
    assert s["blocks"] >= 3
    if r == R:
        assert s["head_and_tail_groups"] >= 1
        assert s["blocks_without_cut"] >= 1
    assert 24 in DIMS and 24 % W.lanes(24) != 0   # a partial last d step


@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("corrupt", [False, True])
def test_sums_are_exact_in_fp32(identity, corrupt):
    """Every partial sum of a row is bounded by the sum of magnitudes,
    which stays below 2**24 quarters: fp32 addition of multiples of 1/4
    is then exact in any order and grouping."""
    names = list(W.patterns(R, W.span_of(R, 16)))
    for name in (["mixed"] if corrupt else names):
        for dim in ((8, 16) if not corrupt else (16,)):
            p = W.bwd_problem(name, R, dim, identity, corrupt)
            assert int(p["mag4"].max()) < 2 ** 24
            assert int(p["g_int"].abs().max()) <= 4   # exact in bf16
            assert torch.equal(p["g_int"].to(torch.bfloat16).long(),
                               p["g_int"])
    for r in W.R_SWEEP:
        p = W.bwd_problem("mixed", r, 16, True)
        assert int(p["mag4"].max()) < 2 ** 24


def test_corrupt_problem():
    p = W.bwd_problem("mixed", R, 16, True, True)
    n_all = p["order"].numel()
    assert n_all == p["inverse"].numel() == p["nnz"] + 11
    assert bool((p["order"][p["nnz"]:] == -1).all())
    bad = p["inverse"] >= p["m_rows"]
    assert int(bad.sum()) == 1 and int(p["counts"][p["bad_key"]]) == 1
    assert bool((p["ref4"][p["bad_key"]] == 0).all())
    # the skipped occurrence sits between two live ones, inside a block
    k_bad = int((p["order"] == int(bad.nonzero())).nonzero())
    assert 0 < k_bad < p["nnz"] - 1


def test_key_cases():
    cases = W.key_cases()
    k, _ = cases["hot_key_two_waves"]
    assert k.numel() == 200 and k.numel() % W.WAVE != 0
    assert int((k[:W.WAVE] == 31337).sum()) == 40
    assert int((k[W.WAVE:2 * W.WAVE] == 31337).sum()) >= 1
    k, _ = cases["equal_below_bit_48"]
    assert k.numel() == W.WAVE and torch.unique(k).numel() == 26
    assert torch.unique(k & ((1 << 48) - 1)).numel() == 1
    assert torch.unique(k & 0xFFFFFFFF).numel() == 1
    ids, _ = cases["matrix_same_id"]
    comp = W.composite_keys(ids)
    u, c = torch.unique(comp, return_counts=True)
    assert u.numel() == 26 and bool((c == 5).all())
    assert torch.unique(comp[:W.WAVE] >> W.KEY_BITS).numel() == 13
    k, _ = cases["pads"]
    assert int(k[0]) == W.PAD_KEY and int(k[1]) == 777
    pads_in_group = (k[:20] == W.PAD_KEY).nonzero().flatten().tolist()
    assert pads_in_group == [0, 4, 5, 13]
    assert bool((k[W.WAVE:2 * W.WAVE] == W.PAD_KEY).all())
    assert k.numel() % W.WAVE != 0
