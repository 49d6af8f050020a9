"""Flagship benchmark: DLRM training on Criteo-TB-shaped synthetic data.

Metric (BASELINE.json): samples/sec (whole node) DLRM at 1/2/4/8 MI355X.
Weak scaling: per-GPU batch is fixed (default 8192, the reference's GPU
benchmark batch size, modelzoo/benchmark/gpu/config.yaml), so value is the
aggregate samples/sec over all ranks.

Launch (single GPU):   python bench.py --steps 50 --warmup 10
Launch (N GPUs): python -m torch.distributed.run --nnodes=1 \
    --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run sets up, warms up, times --steps steps and prints one JSON
result line. --dump-outputs DIR also writes a timed step's loss and logits
as DIR/<name>.npy (the inputs are seeded, so two builds can be compared
output for output; see the option's help for which step). Anything the benchmark measures beyond the
headline figure belongs behind --full (nothing today).
"""
import argparse
import json
import os
import time

import torch

DLRM_BASELINE_SAMPLES_SEC = 141266.06  # DeepRec DLRM FP32+BF16
DUMP_MAX_BYTES = 64 << 20  # --dump-outputs budget over all arrays


def _dump_outputs(directory, outputs, rank):
    """Write each output as <name>.npy (float32); ranks above 0 add a
    _rank<r> suffix. An output over its share of the budget is cut to a
    fixed, seeded sample of its elements."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    per_array = DUMP_MAX_BYTES // max(len(outputs), 1) // 4
    for name, t in outputs.items():
        a = t.detach().to("cpu", torch.float32).numpy()
        if a.size > per_array:
            idx = np.random.default_rng(0).choice(a.size, per_array,
                                                  replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        suffix = f"_rank{rank}" if rank else ""
        np.save(os.path.join(directory, f"{name}{suffix}.npy"), a)


def _snapshot_device_state(device):
    """Byte copies of every live tensor storage on `device`, as
    (view, copy) pairs; _restore_device_state writes them back in place.
    A captured step reads and writes device memory only, so this is all
    the state a replay depends on."""
    import gc
    seen, snap = set(), []
    for o in gc.get_objects():
        if type(o) not in (torch.Tensor, torch.nn.Parameter):
            continue
        if o.device != device:
            continue
        st = o.untyped_storage()
        if st.nbytes() == 0 or st.data_ptr() in seen:
            continue
        seen.add(st.data_ptr())
        view = torch.empty(0, dtype=torch.uint8, device=device).set_(st)
        snap.append((view, view.clone()))
    return snap


def _restore_device_state(snap):
    with torch.no_grad():
        for view, saved in snap:
            view.copy_(saved)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--optimizer", type=str, default="adamasync")
    p.add_argument("--no-bf16", action="store_true")
    p.add_argument("--hip-graph", action="store_true", default=True,
                   help="capture the steady-state step in a hipGraph "
                        "(replay eliminates launch gaps; the distributed "
                        "step captures too via the padded all-to-all)")
    p.add_argument("--no-hip-graph", dest="hip_graph", action="store_false")
    p.add_argument("--force-dist", action="store_true",
                   help="run the distributed (sharded + RCCL) code path "
                        "even at WORLD_SIZE=1 — exercises the exact "
                        "nccl/RCCL call pattern of a full node on a "
                        "single-GPU lease")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write the loss and logits "
                        "a timed step returned as DIR/<name>.npy (float32): "
                        "the third training step, computed again from "
                        "saved state by the captured graph, in a captured "
                        "single-GPU run (its training steps do not repeat "
                        "bit for bit); the last timed step otherwise. Inputs are seeded, so two "
                        "builds can be compared output for output")
    p.add_argument("--full", action="store_true",
                   help="also run whatever the benchmark measures beyond "
                        "its headline figure (nothing today: a plain run "
                        "already does only set-up, warm-up, the timed "
                        "steps and the result line)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world_size > 1 or args.force_dist
    if args.force_dist and world_size == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29561")

    if args.device:
        device = torch.device(args.device)
    elif torch.cuda.is_available():
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")
    if device.type == "cuda":
        torch.cuda.set_device(device)

    if distributed:
        import torch.distributed as dist
        backend = "nccl" if device.type == "cuda" else "gloo"
        dist.init_process_group(backend=backend, rank=rank,
                                world_size=world_size)

    from deeprec_amd.data.synthetic import CriteoSyntheticDataset
    from deeprec_amd.models.dlrm import DLRM
    from deeprec_amd.optimizers import make_optimizer

    torch.manual_seed(42 + rank)
    bf16 = (not args.no_bf16) and device.type == "cuda"
    use_graph = (args.hip_graph and device.type == "cuda"
                 and args.optimizer == "adamasync")
    ev_option = None
    if use_graph:
        from deeprec_amd.embedding.options import EmbeddingVariableOption
        # no growth can happen inside a captured step: pre-size for the
        # full synthetic id space (distributed ranks also hold slot-less
        # dedup entries for every key they SEE, so entries scale with the
        # full space regardless of world size)
        ev_option = EmbeddingVariableOption(init_capacity=1 << 23)
    model = DLRM(device=device, bf16=bf16, sharded=distributed,
                 ev_option=ev_option)
    ds = CriteoSyntheticDataset(batch_size=args.batch, device=device,
                                seed=1234, rank=rank,
                                matrix_format=True)
    opt_kw = {"graph_safe": True} if use_graph else {}
    opt = make_optimizer(args.optimizer, params=model.parameters(),
                         embedding_variables=model.embedding_variables(),
                         learning_rate=0.001, **opt_kw)
    flat_dense = False
    if use_graph and bf16:
        # ONE fused kernel for the dense Adam update that also emits the
        # bf16 weight shadows; dW/db land directly in its flat grad
        # buffer, so the dense all-reduce is one in-place collective
        from deeprec_amd.ops.dense_adam import use_flat_dense_adam
        flat_dense = use_flat_dense_adam(opt, model)
    if distributed:
        from deeprec_amd.parallel import (DenseGradAllreducer,
                                          broadcast_parameters)
        broadcast_parameters(model.parameters())
        if flat_dense:
            from deeprec_amd.ops.dense_adam import FlatGradAllreducer
            opt._dense.refresh_shadows()  # shadows follow the broadcast
            reducer = FlatGradAllreducer(opt._dense)
        else:
            reducer = DenseGradAllreducer(model.parameters())
        # overlap the dense all-reduce with the sparse applies
        opt.pre_dense_step = reducer.wait
    else:
        reducer = None
    if bf16 and not flat_dense:
        # AFTER the parameter broadcast: the bf16 shadows snapshot the
        # weights at enable time
        from deeprec_amd.ops.fused_mlp import enable_weight_cache
        opt.post_step_hook = enable_weight_cache(model)

    # pre-generate batches outside the timed region (CPU RNG is not the
    # system under test); embedding ids differ per step so hash-table and
    # optimizer work is real every timed step
    n_total = args.warmup + args.steps
    batches = [ds.next_batch() for _ in range(min(n_total, 20))]

    # what the most recent step handed back to its caller (--dump-outputs).
    # Detached: a live reference to an eager step's loss keeps its autograd
    # graph (and AccumulateGrad nodes bound to the default stream) alive
    # into the capture below, whose backward then runs on another stream.
    last = {}

    def eager_step(i):
        dense, sparse, labels = batches[i % len(batches)]
        logits = model(dense, sparse)
        loss = model.loss_fn(logits, labels)
        last["loss"], last["logits"] = loss.detach(), logits.detach()
        opt.zero_grad()
        loss.backward()
        if reducer is not None:
            reducer.allreduce(async_op=True)
        opt.step()
        return loss

    # The bf16 step sums weight gradients with fp32 atomics, so a training
    # run never repeats bit for bit and the difference grows with every
    # step. A captured single-GPU run therefore dumps a step that depends
    # on neither --steps nor --warmup: its third training step, computed
    # after the timed region by the captured graph from the device state
    # saved here after the second (capture needs two eager steps).
    snap = None

    one_step = eager_step
    if use_graph:
      try:
        coll = model.collection
        st = coll.storage
        # capture needs warmed state (optimizer slabs, device beta powers,
        # dense adam state) — always run at least 2 eager steps. For the
        # distributed path the eager steps also OBSERVE the per-peer
        # split sizes that size the padded exchange.
        if distributed:
            for i in range(max(args.warmup, 2)):
                eager_step(i)
            torch.cuda.synchronize()
            # pad cap: worst observed split + 50% headroom (overflow trips
            # engine error 4 and fails loudly after the run). The cap is
            # part of the WIRE SHAPE, so every rank must agree: all-reduce
            # the max over ranks
            cap = int(1.5 * max(coll.observed_max_split(), 1)) + 256
            if world_size > 1:
                import torch.distributed as dist
                t = torch.tensor([cap], dtype=torch.int64, device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                cap = int(t.item())
            coll.enable_graph_mode(expected_entries=1 << 23,
                                   expected_slots=1 << 23, pad_cap=cap)
            st = coll.storage
            st.get_slab("adam_m", coll.dim, 0.0)
            st.get_slab("adam_v", coll.dim, 0.0)
            # one eager padded-protocol step so RCCL communicators for the
            # static splits exist before capture
            eager_step(0)
            torch.cuda.synchronize()
        else:
            st.enable_graph_mode(expected_entries=1 << 23,
                                 expected_slots=1 << 23)
            # optimizer slabs must exist before capture
            st.get_slab("adam_m", coll.dim, 0.0)
            st.get_slab("adam_v", coll.dim, 0.0)
            coll.graph_mode = True
            for i in range(max(args.warmup, 2)):
                eager_step(i)
                if i == 1 and args.dump_outputs:
                    torch.cuda.synchronize()
                    snap = _snapshot_device_state(device)
            torch.cuda.synchronize()
        # static input buffers + whole-step capture (the distributed step
        # records its RCCL all-to-alls/all-reduce into the same graph —
        # shapes are static via the padded exchange)
        sdense, sids, slabels = (t.clone() for t in batches[0])
        graph = torch.cuda.CUDAGraph()
        last.clear()
        opt.zero_grad()
        with torch.cuda.graph(graph):
            logits = model(sdense, sids)
            loss = model.loss_fn(logits, slabels)
            loss.backward()
            if reducer is not None:
                reducer.allreduce(async_op=True)
            opt.step()
        torch.cuda.synchronize()
        # replays write the step's results into these static tensors
        last["loss"], last["logits"] = loss.detach(), logits.detach()
        if rank == 0:
            print("bench: hipGraph capture ok", flush=True)

        def graph_step(i):
            dense, sparse, labels = batches[i % len(batches)]
            sdense.copy_(dense, non_blocking=True)
            sids.copy_(sparse, non_blocking=True)
            slabels.copy_(labels, non_blocking=True)
            graph.replay()
            return loss

        one_step = graph_step
      except Exception as e:  # noqa: BLE001
        # never lose the benchmark to a capture failure
        print(f"hip-graph capture failed ({e}); falling back to eager",
              flush=True)
        use_graph = False
        model.collection.graph_mode = False
        if distributed:
            model.collection._pad_cap = None  # back to the dynamic path
            model.collection.local.graph_mode = False
        for i in range(args.warmup):
            eager_step(i)
      if distributed and world_size > 1:
        # the fallback must be COORDINATED: a rank replaying a captured
        # collective against a rank running the eager path would hang
        import torch.distributed as dist
        ok = torch.tensor([1 if use_graph else 0], device=device)
        dist.all_reduce(ok)
        if int(ok.item()) != world_size and use_graph:
            print("bench: peer rank failed capture; using eager on all",
                  flush=True)
            use_graph = False
            one_step = eager_step
            model.collection.graph_mode = False
            model.collection._pad_cap = None
            model.collection.local.graph_mode = False
    else:
        for i in range(args.warmup):
            one_step(i)

    if rank == 0:
        print(f"bench: warmup done (graph={'on' if use_graph else 'off'})",
              flush=True)
    if distributed:
        import torch.distributed as dist
        dist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    if rank == 0:
        print("bench: timed region start", flush=True)
    t0 = time.perf_counter()
    for i in range(args.steps):
        one_step(args.warmup + i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    if rank == 0:
        print("bench: timed region end", flush=True)
    if distributed:
        import torch.distributed as dist
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if use_graph:
        model.collection.storage._check_error()  # no silent slab overflow

    if distributed:
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if device.type == "cuda" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    n_gpus = world_size if distributed else 1
    global_batch = args.batch * n_gpus
    samples_per_sec = global_batch * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if args.dump_outputs:
        if snap is not None and use_graph:
            _restore_device_state(snap)
            one_step(2)
            torch.cuda.synchronize()
            model.collection.storage._check_error()
        _dump_outputs(args.dump_outputs, last, rank)

    out_json = None
    if rank == 0:
        out_json = json.dumps({
            "metric": "samples/sec (whole node) DLRM Criteo-TB-shaped synthetic",
            "value": samples_per_sec,
            "unit": "samples/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": samples_per_sec / DLRM_BASELINE_SAMPLES_SEC,
            "dtype": "bf16" if bf16 else "fp32",
            # label precision: this is the Criteo-1TB-click-log SCHEMA
            # (26 categorical features, reference HASH_BUCKET_SIZES
            # cardinalities) with zipf ids whose per-feature support is
            # capped at 2^20 — a few GB of live embeddings, NOT a TB-
            # scale table. The >=100 GB engine-resident story is
            # measured separately (tools/large_table_bench.py,
            # profiles/large_table_r02.md).
            "data": "synthetic (Criteo-1TB-click-log schema, zipf ids "
                    "capped at 2^20/feature, random-init weights)",
            "config": {"model": "dlrm", "global_batch": global_batch,
                       "seq_len": 1,
                       "parallelism": f"dp{n_gpus}+ep{n_gpus}"
                       if distributed else "single",
                       "hip_graph": use_graph,
                       "optimizer": args.optimizer,
                       "embedding_dim": 16, "num_tables": 26},
        })
        print(out_json, flush=True)

    if distributed:
        import sys
        sys.stdout.flush()
        if use_graph:
            # destroy the hipGraph while the communicator is still alive:
            # a CUDAGraph destructor running after comm abort/teardown
            # (e.g. at interpreter exit) wedges in hipGraphExecDestroy
            one_step = None  # noqa: F841 (drops the closure's graph ref)
            graph = None  # noqa: F841
            import gc
            gc.collect()
            torch.cuda.synchronize()
        from deeprec_amd.parallel import comm
        comm.shutdown(after_capture=use_graph)


if __name__ == "__main__":
    main()
