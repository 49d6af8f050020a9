"""Embedding lookup front-ends with autograd integration.

Capability parity with the reference's lookup surface
(reference: python/ops/embedding_ops.py — embedding_lookup,
embedding_lookup_sparse, safe_embedding_lookup_sparse,
group_embedding_lookup_sparse). Data flow per lookup:

  unique(ids) -> one hash probe (lookup_or_create -> slots)
    -> fused gather+segment-pool (forward)
    -> fused grad scatter to unique keys (backward)
    -> fused sparse optimizer apply on the same slots (optimizer.step)

The slots returned by the single probe are reused end-to-end — the
reference's `_OPT_KvResourceLookupID/CollectEmbedding` pointer-passing
fusion (ops/kv_variable_ops.cc:636).
"""
from __future__ import annotations

import os
from typing import List, Sequence

import torch

from deeprec_amd.embedding.collection import (prep_backward, row_coeffs,
                                              unique_and_probe)
from deeprec_amd.embedding.ragged import RaggedIds
from deeprec_amd.embedding.variable import (EmbeddingVariable,
                                            get_global_step)
from deeprec_amd.ops import functional as F
from deeprec_amd.ops.common import COMBINER_ID, PAD_KEY


class _PooledLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, ev, uniq, slots, inverse, offsets, row_ids,
                counts, combiner, weights, out_dtype):
        out = ev.storage.pooled_lookup(
            uniq, slots, inverse, offsets, row_ids, combiner, weights,
            out_dtype) if hasattr(ev.storage, "pooled_lookup") else None
        if out is None:
            emb = ev.storage.gather(uniq, slots)
            out = F.pooled_forward(emb, inverse, offsets, row_ids, combiner,
                                   weights, out_dtype)
        ctx.ev = ev
        ctx.combiner = combiner
        ctx.save_for_backward(uniq, slots, inverse, offsets, row_ids, counts)
        ctx.weights = weights
        return out

    @staticmethod
    def backward(ctx, grad_out):
        uniq, slots, inverse, offsets, row_ids, counts = ctx.saved_tensors
        ev = ctx.ev
        if (grad_out.device.type == "cuda"
                and hasattr(ev.storage, "ext") and counts.numel()):
            # chunked CSR backward (atomic-free; zipf/seq-scale safe) —
            # the per-occurrence atomic scatter was 3.1 ms on 400k-unique
            # sequence lookups
            grad_unique = _chunked_ev_backward(
                ev, grad_out, inverse, offsets, row_ids, counts,
                ctx.combiner, ctx.weights)
        elif hasattr(ev.storage, "pooled_grad"):
            grad_unique = ev.storage.pooled_grad(
                grad_out, inverse, offsets, row_ids, uniq.numel(),
                ctx.combiner, ctx.weights)
        else:
            grad_unique = F.pooled_backward(
                grad_out, inverse, offsets, row_ids, uniq.numel(),
                ctx.combiner, ctx.weights)
        ev.accumulate_grad(slots, uniq, grad_unique)
        return (None,) * 11


def _chunked_ev_backward(ev, grad_out, inverse, offsets, row_ids, counts,
                         combiner, weights):
    """The collection's segmented backward with n_tables=1."""
    st = ev.storage
    m = counts.numel()
    weights = weights.float() if weights is not None else None
    order, _ = prep_backward(st, inverse, counts)
    comb = torch.full((1,), COMBINER_ID[combiner], dtype=torch.int32,
                      device=grad_out.device)
    row_coeff = row_coeffs(comb, offsets, row_ids, weights)
    return st.ext.group_pooled_bwd_seg(
        grad_out.contiguous(), order, inverse.to(torch.int32),
        row_ids.to(torch.int32),
        weights if weights is not None else torch.Tensor(),
        row_coeff, m, offsets.numel() - 1, 1, ev.dim, False, 0)


def _drop_positions(sp_ids: RaggedIds, keep: torch.Tensor) -> RaggedIds:
    """New RaggedIds with only the kept positions (offsets rebuilt)."""
    row_ids = sp_ids.row_ids()[keep]
    values = sp_ids.values[keep]
    weights = sp_ids.weights[keep] if sp_ids.weights is not None else None
    lengths = torch.zeros(sp_ids.batch_size, dtype=torch.int64,
                          device=values.device)
    lengths.index_add_(0, row_ids.long(),
                       torch.ones_like(row_ids, dtype=torch.int64))
    offsets = torch.zeros(sp_ids.batch_size + 1, dtype=sp_ids.offsets.dtype,
                          device=values.device)
    offsets[1:] = lengths.cumsum(0)
    return RaggedIds(values, offsets, weights)


def embedding_lookup_sparse(ev: EmbeddingVariable, sp_ids: RaggedIds,
                            combiner: str = "mean",
                            out_dtype=None,
                            train: bool = True) -> torch.Tensor:
    """Pooled lookup: [batch, dim]."""
    from deeprec_amd.parallel.sharded_embedding import (
        ShardedEmbeddingVariable, sharded_embedding_lookup_sparse)
    if isinstance(ev, ShardedEmbeddingVariable):
        return sharded_embedding_lookup_sparse(ev, sp_ids, combiner,
                                               out_dtype, train)
    inv = getattr(ev, "invalid_key", None)
    if inv is not None and bool((sp_ids.values == inv).any()):
        # the EV's "no feature" sentinel: dropped before the lookup —
        # never admitted, never trained, zeros in the pooled output
        # (reference: invalid-key semantics of get_embedding_variable)
        sp_ids = _drop_positions(sp_ids, sp_ids.values != inv)
    # fused hash dedup (sort-free) on the GPU training path; a graph-mode
    # EV takes the sync-free padded form of it
    graph_mode = bool(getattr(ev, "graph_mode", False)) and ev.trainable
    uniq, inverse, counts, slots, _rank, _m = unique_and_probe(
        ev.storage, sp_ids.values, train, graph_mode,
        allow_dedup=ev.trainable
        and not os.environ.get("DEEPREC_AMD_DISABLE_DEDUP"),
        bump_step=not (graph_mode and train)
        or ev.first_lookup_of_step())
    if train and ev._record_sparse_ids:
        ev._recorded_ids.append(uniq.detach())
    row_ids = sp_ids.row_ids()
    if not (train and ev.trainable):
        emb = ev.storage.gather(uniq, slots)
        return F.pooled_forward(emb, inverse, offsets=sp_ids.offsets,
                                row_ids=row_ids, combiner=combiner,
                                weights=sp_ids.weights, out_dtype=out_dtype)
    return _PooledLookup.apply(ev._anchor, ev, uniq, slots,
                               inverse.to(torch.int32),
                               sp_ids.offsets.to(torch.int32),
                               row_ids, counts, combiner, sp_ids.weights,
                               out_dtype)


def safe_embedding_lookup_sparse(ev, sp_ids: RaggedIds, combiner="mean",
                                 out_dtype=None, train=True):
    """Like embedding_lookup_sparse; empty rows yield zeros (already the
    pooled kernels' behavior) and negative ids are dropped.
    (reference: fused_safe_embedding_lookup_sparse, embedding_ops.py:1306)"""
    if bool((sp_ids.values < 0).any()):
        sp_ids = _drop_positions(sp_ids, sp_ids.values >= 0)
    return embedding_lookup_sparse(ev, sp_ids, combiner, out_dtype, train)


class _PaddedSeqLookup(torch.autograd.Function):
    """Unpooled gather over a padded id stream; the backward is the
    segmented scatter with one table and identity rows (batch = nnz), over
    an `order` that lists only the valid occurrences."""

    @staticmethod
    def forward(ctx, anchor, ev, uniq, slots, inverse, order, out_dtype):
        out = ev.storage.seq_gather_pad(uniq, slots, inverse, out_dtype)
        ctx.ev = ev
        ctx.save_for_backward(uniq, slots, inverse, order)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        uniq, slots, inverse, order = ctx.saved_tensors
        ev = ctx.ev
        if grad_out.dtype not in (torch.float32, torch.bfloat16):
            grad_out = grad_out.float()
        none = torch.Tensor()
        grad_unique = ev.storage.ext.group_pooled_bwd_seg(
            grad_out.contiguous(), order, inverse, none, none, none,
            uniq.numel(), inverse.numel(), 1, ev.dim, True, 0)
        ev.accumulate_grad(slots, uniq, grad_unique)
        return (None,) * 7


def masked_padded_lookup(ev, ids: torch.Tensor, pad_id: int, out_dtype=None,
                         train: bool = True) -> torch.Tensor:
    """Padded unpooled lookup by masking: look up `ids[ids != pad_id]` and
    scatter the rows into zeros. Shapes depend on the data (a host sync on
    GPU), so it cannot be captured; it runs on every storage and is the
    reference for the static-shape path of `embedding_lookup`."""
    flat = ids.reshape(-1)
    mask = flat != pad_id
    rows = embedding_lookup(ev, flat[mask], out_dtype=out_dtype, train=train)
    emb = torch.zeros(flat.numel(), ev.dim, device=flat.device,
                      dtype=rows.dtype)
    emb = emb.index_put((mask.nonzero().squeeze(1),), rows)
    return emb.reshape(*ids.shape, ev.dim)


def _static_padded_lookup(ev, ids, pad_id, out_dtype, train):
    """HIP-engine path of embedding_lookup(pad_id=...): every shape is a
    function of ids.shape alone."""
    st = ev.storage
    flat = ids.reshape(-1).to(torch.int64)
    n = flat.numel()
    is_pad = flat == pad_id
    # padding becomes the engine's reserved non-key: pass A skips it, pass
    # C gives it inverse -1, so it never reaches the table or a counter
    keys = torch.where(is_pad, torch.full_like(flat, PAD_KEY), flat)
    if not (train and ev.trainable):
        # inference: per-occurrence read-only probe, no insert
        slots = st.lookup(keys)
        inverse = torch.where(
            is_pad, torch.full((n,), -1, dtype=torch.int32,
                               device=flat.device),
            torch.arange(n, dtype=torch.int32, device=flat.device))
        out = st.seq_gather_pad(keys, slots, inverse, out_dtype)
        return out.reshape(*ids.shape, ev.dim)
    if ev.graph_mode:
        d = st.dedup_lookup_capture(
            keys, pad=True, bump_step=ev.first_lookup_of_step())
    else:
        d = st.dedup_lookup(keys, get_global_step(), pad=True)
    if ev._record_sparse_ids:
        if d.m_dev is not None:
            raise RuntimeError(
                "sparse-id recording needs the exact unique keys; "
                "graph_mode pads them")
        ev._recorded_ids.append(d.uniq.detach())
    m = d.counts.numel()
    bounds = torch.zeros(m + 1, dtype=torch.int32, device=flat.device)
    bounds[1:] = d.counts.cumsum(0)
    order = st.ext.csr_scatter_pad(d.inverse, d.rank, bounds, st.error_flag)
    out = _PaddedSeqLookup.apply(ev._anchor, ev, d.uniq, d.slots, d.inverse,
                                 order, out_dtype)
    return out.reshape(*ids.shape, ev.dim)


def embedding_lookup(ev: EmbeddingVariable, ids: torch.Tensor,
                     out_dtype=None, train: bool = True,
                     pad_id=None) -> torch.Tensor:
    """Unpooled lookup: ids [..., ] -> [..., dim] (sequence features).

    With `pad_id`, positions equal to it are padding: zero rows in the
    output, never admitted, never counted in frequency or version, no
    gradient, absent from recorded sparse ids and from `ev.size()`. No
    shape depends on how many there are. On the HIP engine this is a
    static-shape path (padded dedup, pad-aware gather, segmented grad
    scatter) that a graph-mode EV runs without a host sync; on CPU,
    multi-tier and engine-less storages it is `masked_padded_lookup`."""
    if pad_id is not None:
        st = getattr(ev, "storage", None)
        if (isinstance(ev, EmbeddingVariable) and ev.device.type == "cuda"
                and hasattr(st, "ext") and not hasattr(st, "apply_split")):
            return _static_padded_lookup(ev, ids, pad_id, out_dtype, train)
        return masked_padded_lookup(ev, ids, pad_id, out_dtype, train)
    flat = ids.reshape(-1)
    n = flat.numel()
    offsets = torch.arange(n + 1, dtype=torch.int32, device=flat.device)
    out = embedding_lookup_sparse(
        ev, RaggedIds(flat, offsets), combiner="sum",
        out_dtype=out_dtype, train=train)
    return out.reshape(*ids.shape, ev.dim)


def group_embedding_lookup_sparse(evs: Sequence[EmbeddingVariable],
                                  sp_ids_list: Sequence[RaggedIds],
                                  combiners=None, out_dtype=None,
                                  train: bool = True) -> List[torch.Tensor]:
    """N lookups in one call (reference: GroupEmbeddingVarLookup,
    ops/kv_variable_ops.cc:404). Loops over the tables; the fused
    multi-table path is EmbeddingCollection."""
    if combiners is None:
        combiners = ["mean"] * len(evs)
    if len(evs) != len(sp_ids_list) or len(evs) != len(combiners):
        raise ValueError("group_embedding_lookup_sparse: length mismatch")
    return [embedding_lookup_sparse(ev, sp, c, out_dtype, train)
            for ev, sp, c in zip(evs, sp_ids_list, combiners)]
