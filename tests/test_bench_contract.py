"""bench.py driver contract: ONE parseable JSON line with the required
fields, single-process and through a real 2-rank torchrun gloo launch
(the CPU analog of the driver's BENCH/SCALE runs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _last_json(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines, f"no JSON line in output:\n{stdout[-500:]}"
    return json.loads(lines[-1])


def test_bench_single_process_contract():
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "256", "--no-hip-graph"],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    d = _last_json(r.stdout)
    assert REQUIRED <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["config"]["model"] == "dlrm"
    assert abs(d["value"] - d["config"]["global_batch"] * 1000.0
               / d["ms_per_step"]) / d["value"] < 1e-6


def test_bench_two_rank_gloo_contract():
    """torchrun --nproc-per-node 2: exactly rank 0 prints the JSON,
    n_gpus=2, whole-job value (2x per-rank batch), dp2+ep2 label."""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29574", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--batch", "128"],
        capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-800:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one rank must print the JSON"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["global_batch"] == 256  # whole node, not per rank
    assert d["config"]["parallelism"] == "dp2+ep2"
    assert d["value"] > 0


def test_bench_force_dist_single_process():
    """--force-dist at world=1 on CPU: the sharded+collective code path
    (gloo self-exchange) behind the same JSON contract."""
    r = subprocess.run(
        [sys.executable, "bench.py", "--force-dist", "--steps", "2",
         "--warmup", "1", "--batch", "128"],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    d = _last_json(r.stdout)
    assert d["config"]["parallelism"] == "dp1+ep1"
    assert d["value"] > 0


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's loss and logits as
    float32 .npy; the inputs are seeded, so a second run with the same
    arguments reproduces them. --full is accepted and keeps the contract."""
    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
             "--warmup", "1", "--batch", "64", "--device", "cpu", "--full",
             "--dump-outputs", str(out)],
            capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-800:]
        d = _last_json(r.stdout)
        assert REQUIRED <= set(d) and d["steps"] == 3
        assert sorted(os.listdir(out)) == ["logits.npy", "loss.npy"]
        dumps.append({f: np.load(out / f) for f in os.listdir(out)})
    a, b = dumps
    assert a["logits.npy"].dtype == np.float32
    assert a["loss.npy"].dtype == np.float32
    assert a["logits.npy"].size == 64 and a["loss.npy"].size == 1
    assert np.isfinite(a["logits.npy"]).all()
    assert np.isfinite(a["loss.npy"]).all()
    for f in a:
        np.testing.assert_array_equal(a[f], b[f])


def _captured_dump(out, steps):
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
         "--warmup", "2", "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    d = _last_json(r.stdout)
    assert d["steps"] == steps and d["config"]["hip_graph"] is True
    return {f: np.load(out / f) for f in ("loss.npy", "logits.npy")}


@pytest.fixture(scope="module")
def one_step_dump(tmp_path_factory):
    return _captured_dump(tmp_path_factory.mktemp("dump1"), 1)


@pytest.mark.gpu
def test_bench_captured_dump_independent_of_steps(one_step_dump, tmp_path):
    """A captured run dumps its third training step, computed again after
    the timed region from the state saved after the second, so the dump of
    a 1500-step run equals that of a 1-step run. (The last step of 1500
    would not: the run overfits its 20 batches and the logits grow to
    tens.) Bound: the logits are bf16, so one bf16 ulp (2^-7 relative) at
    the scale of the largest logit, which is what fp32-atomic summation
    order in the two steps before the saved state can flip; the loss is a
    mean over the batch whose derivative in each logit (sigmoid - label)
    is below 1 in size."""
    ref = one_step_dump
    got = _captured_dump(tmp_path, 1500)
    ulp = 2.0 ** -7 * float(np.abs(ref["logits.npy"]).max())
    assert got["logits.npy"].shape == ref["logits.npy"].shape == (8192,)
    dl = np.abs(got["logits.npy"] - ref["logits.npy"]).max()
    ds = abs(float(got["loss.npy"]) - float(ref["loss.npy"]))
    print(f"max |dlogits| {dl:.3e} (bound {ulp:.3e}), |dloss| {ds:.3e}")
    assert dl <= ulp
    assert ds <= ulp


def test_graft_entry_surface():
    import __graft_entry__
    assert callable(__graft_entry__.build)
    assert callable(__graft_entry__.smoke)
