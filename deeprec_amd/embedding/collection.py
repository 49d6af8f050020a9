"""EmbeddingCollection — N same-dim tables in one physical storage.

The MI355X-first replacement for per-table lookups (reference capability:
GroupEmbeddingVarLookup, ops/kv_variable_ops.cc:404 and the SOK grouped
path): all tables share one hash table + value slab via composite keys
(table_id << KEY_BITS | id), so a training step does ONE unique, ONE hash
probe, ONE fused gather+pool kernel (output [B, N*D], the concat layout
models consume), ONE atomic-free CSR grad scatter and ONE fused optimizer
apply — independent of table count. On the DLRM profile this collapses
~500 kernel launches/step into ~25.

Logical per-table semantics (export/restore/frequency/eviction) are
preserved: composite keys decompose as (table_id, raw_key).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from deeprec_amd.embedding.options import EmbeddingVariableOption
from deeprec_amd.embedding.ragged import RaggedIds
from deeprec_amd.embedding.variable import get_global_step
from deeprec_amd.ops import functional as F
from deeprec_amd.ops.common import COMBINER_ID, KEY_BITS, DedupResult


def unique_and_probe(storage, keys, train: bool, graph_mode: bool = False,
                     allow_dedup: bool = True,
                     bump_step: bool = True) -> DedupResult:
    """unique + single hash probe. GPU training uses the fused hash dedup
    (no sorts) while the storage prefers it; everything else is
    torch.unique + the probe, with rank=None. A storage that can dedup has
    `prefers_dedup` (and with it `dedup_lookup`, `observe_uniq_ratio`);
    one that cannot simply lacks it. bump_step=False (capture only) marks
    a second lookup of the same storage within one step."""
    if graph_mode and train:
        return storage.dedup_lookup_capture(keys, bump_step=bump_step)
    prefers_dedup = getattr(storage, "prefers_dedup", None)
    if train and allow_dedup and prefers_dedup is not None \
            and prefers_dedup():
        return storage.dedup_lookup(keys, get_global_step())
    uniq, inverse, counts = torch.unique(
        keys, return_inverse=True, return_counts=True)
    slots = storage.lookup_or_create(uniq, counts, get_global_step(),
                                     train=train)
    if prefers_dedup is not None:
        storage.observe_uniq_ratio(uniq.numel(), keys.numel())
    return DedupResult(uniq, inverse.to(torch.int32), counts, slots, None,
                       None)


def prep_backward(storage, inverse, counts, rank=None):
    """CSR over unique keys: `order` lists the occurrences sorted by
    unique row, which is what the occurrence-balanced backward walks.
    `rank` is the DedupResult.rank that came with this `inverse`."""
    m = counts.numel()
    c32 = counts.to(torch.int32)
    if inverse.device.type != "cuda":
        bounds = torch.zeros(m + 1, dtype=torch.int32, device=inverse.device)
        bounds[1:] = c32.cumsum(0)
        order = torch.argsort(inverse.long()).to(torch.int32)
        return order, bounds
    # int32 scan in two launches of ours (was: fill, rocprim scan, cast)
    bounds = storage.ext.csr_bounds(c32.contiguous())
    if rank is not None:
        # pass C already recorded each occurrence's rank within its key,
        # so order is a direct scatter (no atomic-cursor pass over nnz)
        order = storage.ext.csr_scatter(inverse, rank, bounds,
                                        storage.error_flag)
    else:  # torch.unique (sort) path
        order = storage.ext.csr_order(inverse, bounds, m)
    return order, bounds


def row_coeffs(comb, offsets, row_ids, weights):
    """Combiner coefficient per pooled row. `comb` holds the combiner id
    of each row (or one id, broadcast); `weights` is fp32 or None."""
    lengths = (offsets[1:] - offsets[:-1]).float()
    if weights is None:
        wsum = lengths
        wsq = lengths
    else:
        wsum = torch.zeros_like(lengths)
        wsum.index_add_(0, row_ids.long(), weights)
        wsq = torch.zeros_like(lengths)
        wsq.index_add_(0, row_ids.long(), weights * weights)
    denom = torch.where(comb == 2, wsq.sqrt(), wsum)
    coeff = torch.where(comb == 0, torch.ones_like(denom),
                        1.0 / denom.clamp(min=1e-12))
    # empty rows get 0 under every combiner; no occurrence reads it
    return torch.where(lengths > 0, coeff, torch.zeros_like(coeff))


class EmbeddingCollection:
    def __init__(self, name: str, table_names: Sequence[str],
                 embedding_dim: int,
                 ev_option: Optional[EmbeddingVariableOption] = None,
                 combiners=None, device=None, value_dtype=torch.float32,
                 generator=None, trainable: bool = True):
        self.name = name
        self.table_names = list(table_names)
        self.n_tables = len(self.table_names)
        assert 0 < self.n_tables < (1 << (63 - KEY_BITS))
        self.dim = embedding_dim
        self.device = torch.device(device or "cpu")
        self.trainable = trainable
        self.ev_option = ev_option or EmbeddingVariableOption()
        self.combiners = list(combiners or ["mean"] * self.n_tables)
        assert len(self.combiners) == self.n_tables

        # one storage; default matrix holds n_tables blocks of dvd rows
        import copy
        opt = copy.deepcopy(self.ev_option)
        dvd = max(1, opt.init_option.default_value_dim)
        opt.init_option.default_value_dim = dvd * self.n_tables
        from deeprec_amd.embedding.options import StorageType
        fp8 = opt.storage_option.storage_type == StorageType.HBM_FP8
        if fp8:
            from deeprec_amd.ops.quant_backend import (QuantizedHbmStorage,
                                                       require_cuda_for_fp8)
            require_cuda_for_fp8(self.device, f"EmbeddingCollection {name!r}")
            self.trainable = trainable = False
            self.storage = QuantizedHbmStorage(embedding_dim, opt,
                                               value_dtype, self.device,
                                               generator)
        elif self.device.type == "cuda":
            from deeprec_amd.ops.hip_backend import HbmStorage
            self.storage = HbmStorage(embedding_dim, opt, value_dtype,
                                      self.device, generator)
        else:
            from deeprec_amd.ops.cpu_backend import CpuStorage
            self.storage = CpuStorage(embedding_dim, opt, value_dtype,
                                      self.device, generator)
        self.storage.key_bits = KEY_BITS
        self.storage.dvd_per_table = dvd
        self._combiner_ids = torch.tensor(
            [COMBINER_ID[c] for c in self.combiners], dtype=torch.int32,
            device=self.device)
        self._anchor = torch.zeros((), device=self.device,
                                   requires_grad=trainable)
        self._matrix_cache = {}
        self.graph_mode = False
        self._pending_grads: List = []
        self._recorded_ids: List[torch.Tensor] = []
        self._record_sparse_ids = False

    # ---------------- composite key helpers ----------------
    def composite(self, table: int, ids: torch.Tensor) -> torch.Tensor:
        return ids + (table << KEY_BITS)

    def decompose(self, keys: torch.Tensor):
        return keys >> KEY_BITS, keys & ((1 << KEY_BITS) - 1)

    # ---------------- optimizer-facing API (EV-compatible) ----------------
    def accumulate_grad(self, slots, keys, grad_unique):
        self._pending_grads.append((slots, keys, grad_unique))

    def consume_grads(self):
        out = self._pending_grads
        self._pending_grads = []
        return out

    def get_slab(self, name, width=None, init_value=0.0, dtype=torch.float32):
        return self.storage.get_slab(name, width or self.dim, init_value,
                                     dtype)

    def size(self):
        return self.storage.size()

    def total_count(self):
        return self.storage.total_count()

    # ---------------- lookup ----------------
    def _concat_inputs(self, sp_list: Sequence[RaggedIds]):
        batch = sp_list[0].batch_size
        dev = self.device
        vals, offs, rows, weights = [], [], [], []
        base = 0
        any_weights = any(sp.weights is not None for sp in sp_list)
        for t, sp in enumerate(sp_list):
            assert sp.batch_size == batch, "collection: batch mismatch"
            vals.append(sp.values + (t << KEY_BITS))
            o = sp.offsets.to(torch.int64)
            offs.append((o[:-1] if t + 1 < len(sp_list) else o) + base)
            base += int(sp.values.numel())
            rows.append(sp.row_ids().to(torch.int64) + t * batch)
            if any_weights:
                weights.append(sp.weights.float() if sp.weights is not None
                               else torch.ones(sp.values.numel(), device=dev))
        values_cat = torch.cat(vals)
        offsets_cat = torch.cat(offs).to(torch.int32)
        row_ids_cat = torch.cat(rows).to(torch.int32)
        weights_cat = torch.cat(weights) if any_weights else None
        return batch, values_cat, offsets_cat, row_ids_cat, weights_cat

    def _row_coeffs(self, offsets_cat, row_ids_cat, weights_cat, batch):
        """[N*B] combiner coefficient per pooled row."""
        return row_coeffs(self._combiner_ids.repeat_interleave(batch),
                          offsets_cat, row_ids_cat, weights_cat)

    def lookup(self, sp_list: Sequence[RaggedIds], out_dtype=None,
               train: bool = True) -> torch.Tensor:
        """-> [batch, n_tables * dim] pooled embeddings (concat layout)."""
        assert len(sp_list) == self.n_tables
        batch, values_cat, offsets_cat, row_ids_cat, weights_cat = \
            self._concat_inputs(sp_list)
        train = train and self.trainable
        d = self._dedup_and_probe(values_cat, train)
        if not train:
            return self._forward(d.uniq, d.slots, d.inverse, offsets_cat,
                                 weights_cat, batch, out_dtype)
        order, bounds = self._prep_backward(d.inverse, d.counts, d.rank)
        row_coeff = self._row_coeffs(offsets_cat, row_ids_cat, weights_cat,
                                     batch)
        return _CollectionLookup.apply(
            self._anchor, self, d.uniq, d.slots, d.inverse, offsets_cat,
            row_ids_cat, order, bounds, row_coeff, weights_cat, batch,
            out_dtype, False)

    def _dedup_and_probe(self, values_cat, train) -> DedupResult:
        d = unique_and_probe(self.storage, values_cat, train,
                             self.graph_mode)
        if train and self._record_sparse_ids:
            self._recorded_ids.append(d.uniq.detach())
        return d

    def _prep_backward(self, inverse, counts, rank=None):
        return prep_backward(self.storage, inverse, counts, rank)

    def matrix_inputs(self, ids: torch.Tensor):
        """(values_cat, offsets, row_ids, row_coeff) for ids [batch,
        n_tables], one id per table per sample. Everything but the
        tagged keys is cached per batch size."""
        offsets, row_ids, row_coeff, tags = self._matrix_static(ids)
        return ids.t().reshape(-1) + tags, offsets, row_ids, row_coeff

    def _matrix_static(self, ids: torch.Tensor):
        """(offsets, row_ids, row_coeff, tags): the part of matrix_inputs
        that depends on the batch size alone."""
        batch, n = ids.shape
        assert n == self.n_tables
        cache = self._matrix_cache.get(batch)
        if cache is None:
            dev = self.device
            nb = n * batch
            cache = (
                torch.arange(nb + 1, dtype=torch.int32, device=dev),
                torch.arange(nb, dtype=torch.int32, device=dev),
                torch.ones(nb, device=dev),
                (torch.arange(n, dtype=torch.int64, device=dev)
                 << KEY_BITS).repeat_interleave(batch))
            self._matrix_cache[batch] = cache
        return cache

    def lookup_matrix(self, ids: torch.Tensor, out_dtype=None,
                      train: bool = True) -> torch.Tensor:
        """Fixed-shape fast path: ids [batch, n_tables] (one id per table
        per sample, the Criteo layout). All ragged glue (offsets, row ids,
        combiner coeffs, table tags) is cached per batch size, so a step
        costs: 1 transpose+add, 1 unique, the probe, the fused fwd/bwd and
        the apply. A captured training step on a storage that offers
        dedup_lookup_capture_matrix skips the transpose+add as well: pass A
        forms the composite keys from `ids` itself."""
        batch = ids.shape[0]
        train = train and self.trainable
        if (train and self.graph_mode and not self._record_sparse_ids
                and ids.dtype == torch.int64 and ids.is_contiguous()
                and hasattr(self.storage, "dedup_lookup_capture_matrix")):
            offsets, row_ids, row_coeff, _ = self._matrix_static(ids)
            d = self.storage.dedup_lookup_capture_matrix(ids)
        else:
            values_cat, offsets, row_ids, row_coeff = self.matrix_inputs(ids)
            d = self._dedup_and_probe(values_cat, train)
        if not train:
            return self._forward(d.uniq, d.slots, d.inverse, offsets, None,
                                 batch, out_dtype)
        order, bounds = self._prep_backward(d.inverse, d.counts, d.rank)
        return _CollectionLookup.apply(
            self._anchor, self, d.uniq, d.slots, d.inverse, offsets,
            row_ids, order, bounds, row_coeff, None, batch, out_dtype, True)

    def _forward(self, uniq, slots, inverse, offsets_cat, weights_cat, batch,
                 out_dtype, emb_override=None):
        # serving storages without the HIP engine (CPU-offloaded or
        # remote-KV rows under a CUDA model) take the generic gather+pool
        # path below — it is pure torch and runs on either device
        if self.device.type == "cuda" and hasattr(self.storage, "ext"):
            if emb_override is not None:
                return self.storage.ext.group_pooled_fwd_direct(
                    emb_override.contiguous(), uniq, inverse, offsets_cat,
                    weights_cat if weights_cat is not None
                    else torch.Tensor(),
                    self._combiner_ids, batch, self.n_tables,
                    out_dtype or torch.float32)
            return self.storage.group_pooled_lookup(
                uniq, slots, inverse, offsets_cat, weights_cat,
                self._combiner_ids, batch, self.n_tables, out_dtype)
        # CPU reference: gather then pool per-table slices
        emb = (emb_override if emb_override is not None
               else self.storage.gather(uniq, slots))  # [m, D]
        outs = []
        row_ids_all = None
        nb = offsets_cat.numel() - 1  # == n_tables * batch
        lengths = (offsets_cat[1:] - offsets_cat[:-1]).long()
        row_ids_cat = torch.repeat_interleave(
            torch.arange(nb, dtype=torch.int64,
                         device=offsets_cat.device), lengths)
        for t in range(self.n_tables):
            lo, hi = t * batch, (t + 1) * batch
            jmask = (row_ids_cat >= lo) & (row_ids_cat < hi)
            sub_off = (offsets_cat[lo:hi + 1] - offsets_cat[lo]).to(
                torch.int32)
            out_t = F.pooled_forward(
                emb, inverse[jmask], sub_off,
                (row_ids_cat[jmask] - lo).to(torch.int32),
                self.combiners[t],
                weights_cat[jmask] if weights_cat is not None else None,
                out_dtype)
            outs.append(out_t)
        return torch.cat(outs, dim=1)  # [B, N*D], table-major inner

    def _backward(self, grad_out, order, bounds, inverse, row_ids_cat,
                  weights_cat, row_coeff, m, batch, identity_rows=False):
        """grad_unique [m, dim]. `inverse` is the occurrence -> unique-row
        map `order` was built from (the GPU kernel walks occurrences and
        needs no bounds; the CPU reference uses bounds)."""
        if self.device.type == "cuda":
            # occurrence-balanced: cost depends on nnz only, so neither
            # key skew nor an nnz-padded m (graph capture) changes it
            return self.storage.ext.group_pooled_bwd_seg(
                grad_out.contiguous(), order, inverse, row_ids_cat,
                weights_cat if weights_cat is not None else torch.Tensor(),
                row_coeff, m, batch, self.n_tables, self.dim,
                identity_rows, 0)
        # CPU reference path
        g = grad_out.float().reshape(batch, self.n_tables, self.dim)
        grad_unique = torch.zeros(m, self.dim)
        order_l = order.long()
        j_sorted = order_l
        # expand bounds to per-occurrence unique index
        counts = (bounds[1:] - bounds[:-1]).long()
        u_of_k = torch.repeat_interleave(
            torch.arange(m, dtype=torch.int64), counts)
        rid = row_ids_cat.long()[j_sorted]
        t_idx = rid // batch
        b_idx = rid % batch
        contrib = g[b_idx, t_idx, :] * row_coeff[rid].unsqueeze(1)
        if weights_cat is not None:
            contrib = contrib * weights_cat[j_sorted].unsqueeze(1)
        grad_unique.index_add_(0, u_of_k, contrib)
        return grad_unique

    # ---------------- checkpoint / maintenance ----------------
    def export(self, include_filtered: bool = False):
        """Whole-collection export with composite keys (checkpoint format);
        per-table views come from export_tables()."""
        return self.storage.export(include_filtered)

    def restore(self, keys, values, freqs=None, versions=None):
        self.storage.import_(keys.to(self.device), values, freqs, versions)

    def export_tables(self, include_filtered: bool = False):
        """-> dict table_name -> (keys, values, freqs, versions)."""
        keys, values, freqs, versions = self.storage.export()
        tid, raw = self.decompose(keys)
        out = {}
        for t, name in enumerate(self.table_names):
            mask = tid == t
            out[name] = (raw[mask], values[mask], freqs[mask],
                         versions[mask])
        return out

    def restore_table(self, table: int, keys, values, freqs=None,
                      versions=None):
        self.storage.import_(self.composite(table, keys.to(self.device)),
                             values, freqs, versions)

    def shrink(self, step: Optional[int] = None) -> int:
        return self.storage.shrink(
            step if step is not None else get_global_step())

    def start_sparse_recording(self):
        self._record_sparse_ids = True

    def consume_recorded_ids(self) -> torch.Tensor:
        if not self._recorded_ids:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        ids = torch.unique(torch.cat(self._recorded_ids))
        self._recorded_ids = []
        return ids

    def get_frequency(self, table: int, keys):
        return self.storage.frequencies(
            self.composite(table, keys.to(self.device)))

    def get_version(self, table: int, keys):
        return self.storage.versions(
            self.composite(table, keys.to(self.device)))

    def __repr__(self):
        return (f"EmbeddingCollection(name={self.name!r}, "
                f"tables={self.n_tables}, dim={self.dim}, "
                f"device={self.device})")


class _CollectionLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, coll, uniq, slots, inverse, offsets_cat,
                row_ids_cat, order, bounds, row_coeff, weights_cat, batch,
                out_dtype, identity_rows=False):
        out = coll._forward(uniq, slots, inverse, offsets_cat, weights_cat,
                            batch, out_dtype)
        ctx.coll = coll
        ctx.batch = batch
        ctx.identity_rows = identity_rows
        ctx.save_for_backward(uniq, slots, order, bounds, inverse,
                              row_ids_cat, row_coeff)
        ctx.weights_cat = weights_cat
        return out

    @staticmethod
    def backward(ctx, grad_out):
        uniq, slots, order, bounds, inverse, row_ids_cat, row_coeff = \
            ctx.saved_tensors
        coll = ctx.coll
        grad_unique = coll._backward(grad_out, order, bounds, inverse,
                                     row_ids_cat, ctx.weights_cat,
                                     row_coeff, uniq.numel(), ctx.batch,
                                     ctx.identity_rows)
        coll.accumulate_grad(slots, uniq, grad_unique)
        # the anchor only ties this node into the graph; it has no gradient
        return (None,) * 14
