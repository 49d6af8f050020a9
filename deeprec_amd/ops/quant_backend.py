"""fp8-resident HBM storage: an inference-only HbmStorage whose value slab
is OCP e4m3 bytes with one fp32 scale per row.

Rows cost dim + 4 bytes instead of 4 * dim (20 B instead of 64 B at dim
16) and are dequantized inside the gather/pool kernels
(Q8Rows, ops/hip/ev_read_kernels.hip): value(s, d) = fl32(scale[s] *
decode_e4m3(q[s, d])), exactly ops/fp8.dequantize_fp8_rows. The hash table,
admission metadata and default_values (fp32, small) are HbmStorage's own.
Quantization is the per-row scheme of ops/fp8.py (scale = amax/448, 1 for
an all-zero row), applied by the existing quant_rows_e4m3 kernel as rows
are imported; the file format of tools/quantize_embeddings.py --format fp8
loads without requantizing through import_quantized().

Reached through StorageType.HBM_FP8, ops.fp8.quantize_embeddings_fp8()
(post-training, in place) and Predictor(fp8_embeddings=True). int8 rows
stay a file format of the quantize tool; only e4m3 is served resident.
"""
from __future__ import annotations

import torch

from deeprec_amd.ops.common import COMBINER_ID, KEY_BITS
from deeprec_amd.ops.fp8 import dequantize_fp8_rows
from deeprec_amd.ops.hip_backend import HbmStorage

# rows quantized per step of an import or a conversion: bounds the fp32
# staging on the device (64 MB at dim 16) whatever the table size
_CHUNK_ROWS = 1 << 20


def require_cuda_for_fp8(device, who: str):
    if torch.device(device).type != "cuda":
        raise NotImplementedError(
            f"{who}: StorageType.HBM_FP8 is served by the gfx950 "
            f"dequantizing kernels and needs a CUDA device, not "
            f"{torch.device(device).type!r} (there is no CPU emulation of "
            "the quantized storage)")


def _inference_only(what: str):
    def method(self, *a, **kw):
        raise RuntimeError(
            f"{what} is not supported by {type(self).__name__}: the "
            "storage is inference-only (rows are e4m3 bytes; nothing can "
            "train or admit into it)")
    method.__name__ = what
    return method


class QuantizedHbmStorage(HbmStorage):
    """HbmStorage with `values` uint8 [slots, dim] (e4m3) and `scales`
    fp32 [slots]. Lookups are pure finds; rows arrive through import_ /
    import_quantized only."""

    inference_only = True

    # ---------------- allocation ----------------
    def _alloc_slabs(self, max_slots: int):
        # zero bytes / unit scales: a never-written row decodes to zeros
        self.values = torch.zeros(max_slots, self.dim, dtype=torch.uint8,
                                  device=self.device)
        self.scales = torch.ones(max_slots, dtype=torch.float32,
                                 device=self.device)

    def _grow_slots(self, need: int):
        old = self.max_slots
        new_cap = old
        while new_cap < need:
            new_cap *= 2
        values, scales = self.values, self.scales
        self._alloc_slabs(new_cap)
        self.values[:old] = values
        self.scales[:old] = scales

    @classmethod
    def from_storage(cls, src: HbmStorage) -> "QuantizedHbmStorage":
        """Take over a trained HbmStorage: the hash-table arrays and
        counters as they are, the value rows quantized chunk by chunk. The
        source's fp32 slab and optimizer slabs are dropped."""
        self = cls.__new__(cls)
        self.__dict__.update(
            (k, v) for k, v in src.__dict__.items()
            if k not in ("values", "slabs", "_slab_init", "graph_mode",
                         "_epoch_dev", "_step_dev"))
        self.slabs = {}
        self._slab_init = {}
        self._alloc_slabs(src.max_slots)
        src._sync_counters()
        n = src._slots_hint
        self._slots_hint, self._entries_hint = n, src._entries_hint
        for lo in range(0, n, _CHUNK_ROWS):
            hi = min(n, lo + _CHUNK_ROWS)
            q, s = self.ext.quant_rows_e4m3(src.values[lo:hi])
            self.values[lo:hi] = q
            self.scales[lo:hi] = s
        src.values = None
        src.slabs = {}
        return self

    # ---------------- training entry points ----------------
    get_slab = _inference_only("get_slab")
    enable_graph_mode = _inference_only("enable_graph_mode")
    dedup_lookup = _inference_only("dedup_lookup")
    dedup_lookup_capture = _inference_only("dedup_lookup_capture")
    dedup_only_capture = _inference_only("dedup_only_capture")
    dedup_lookup_capture_owner = _inference_only("dedup_lookup_capture_owner")
    _dedup_claim = _inference_only("_dedup_claim")
    _dedup_count = _inference_only("_dedup_count")
    _dedup_admit = _inference_only("_dedup_admit")

    def lookup_or_create(self, keys, counts, step, train=True):
        if train:
            _inference_only("lookup_or_create(train=True)")(self)
        return self.lookup(keys)

    # ---------------- reads ----------------
    def gather(self, keys, slots, out_dtype=None):
        return self.ext.ev_gather_q8(
            self.values, self.scales, self.default_values, keys, slots,
            self._no_permission_value(), self._use_no_permission(),
            out_dtype or torch.float32)

    def seq_gather_pad(self, keys, slots, inverse, out_dtype=None):
        return self.ext.seq_gather_pad_q8(
            self.values, self.scales, self.default_values, keys, slots,
            inverse, self._no_permission_value(), self._use_no_permission(),
            out_dtype or torch.float32)

    def pooled_lookup(self, keys, slots, inverse, offsets, row_ids, combiner,
                      weights, out_dtype):
        return self.ext.pooled_fwd_q8(
            self.values, self.scales, self.default_values, keys, slots,
            inverse.to(torch.int32), offsets.to(torch.int32),
            weights.float() if weights is not None else torch.Tensor(),
            COMBINER_ID[combiner], self._no_permission_value(),
            self._use_no_permission(), out_dtype or torch.float32)

    def group_pooled_lookup(self, keys, slots, inverse, offsets, weights,
                            combiner_ids, batch, n_tables, out_dtype):
        return self.ext.group_pooled_fwd_q8(
            self.values, self.scales, self.default_values, keys, slots,
            inverse, offsets,
            weights if weights is not None else torch.Tensor(),
            combiner_ids, batch, n_tables, KEY_BITS,
            self._no_permission_value(), self._use_no_permission(),
            out_dtype or torch.float32)

    # ---------------- import / export ----------------
    def import_(self, keys, values, freqs=None, versions=None,
                slab_rows=None):
        """Quantize fp32 rows and store them; existing keys keep their
        slots (delta updates overwrite in place). Rows are staged on the
        device in chunks, so `values` may be a CPU tensor of any size.
        slab_rows is ignored: there is no optimizer state here."""
        m = keys.numel()
        for lo in range(0, m, _CHUNK_ROWS):
            hi = min(m, lo + _CHUNK_ROWS)
            q, s = self.ext.quant_rows_e4m3(
                values[lo:hi].to(self.device, torch.float32).contiguous())
            self.import_quantized(
                keys[lo:hi], q, s,
                freqs[lo:hi] if freqs is not None else None,
                versions[lo:hi] if versions is not None else None)

    def import_quantized(self, keys, q, scale, freqs=None, versions=None):
        """Store e4m3 bytes [m, dim] and fp32 scales [m] unchanged."""
        m = keys.numel()
        if m == 0:
            return
        if q.dtype != torch.uint8 or tuple(q.shape) != (m, self.dim) \
                or scale.numel() != m:
            raise ValueError(
                f"import_quantized: want uint8 [{m}, {self.dim}] bytes and "
                f"{m} scales, got {q.dtype} {tuple(q.shape)} and "
                f"{scale.numel()} scales")
        slots = self._import_entries(keys.to(self.device), freqs,
                                     versions).long()
        self.values[slots] = q.to(self.device)
        self.scales[slots] = scale.to(self.device, torch.float32)
        self._check_error()
        self._sync_counters()

    def export(self, include_filtered: bool = False):
        """(keys, dequantized fp32 rows, freqs, versions) — the checkpoint
        format, so Saver works unchanged."""
        keys, slots, freqs, versions = self._export_entries()
        adm = slots >= 0
        s = slots[adm].long()
        out = (keys[adm], dequantize_fp8_rows(self.values[s], self.scales[s]),
               freqs[adm].to(torch.int64), versions[adm])
        if include_filtered:
            out = out + (keys[~adm], freqs[~adm].to(torch.int64))
        return out

    def export_quantized(self):
        """(keys, e4m3 bytes, scales, freqs, versions) of admitted keys."""
        keys, slots, freqs, versions = self._export_entries()
        adm = slots >= 0
        s = slots[adm].long()
        return (keys[adm], self.values[s], self.scales[s],
                freqs[adm].to(torch.int64), versions[adm])

    # ---------------- maintenance ----------------
    def _row_norms(self, slots):
        return dequantize_fp8_rows(self.values[slots],
                                   self.scales[slots]).norm(dim=1)

    def _rebuild(self, keys, slots, freqs, versions):
        old_slots = slots[slots >= 0].long()
        self.scales[: old_slots.numel()] = self.scales[old_slots]
        super()._rebuild(keys, slots, freqs, versions)

    def memory_usage(self) -> dict:
        out = super().memory_usage()
        out["scale_bytes"] = self.scales.numel() * self.scales.element_size()
        out["total_bytes"] += out["scale_bytes"]
        return out
