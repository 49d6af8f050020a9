"""The CPU-visible edges of fp8-resident embedding serving: the option
surface and the converter refuse a CPU device by name, the quantize tool's
raw loader round-trips its own file, and the saver keeps optimizer slabs
away from an inference-only storage."""
import sys

import pytest
import torch


def _fp8_option():
    from deeprec_amd.embedding.options import (
        EmbeddingVariableOption, StorageOption, StorageType)
    return EmbeddingVariableOption(
        storage_option=StorageOption(storage_type=StorageType.HBM_FP8))


def test_storage_type_value():
    from deeprec_amd.embedding.options import StorageType
    assert StorageType.HBM_FP8.value == 5


def test_hbm_fp8_on_cpu_raises():
    from deeprec_amd.embedding.collection import EmbeddingCollection
    from deeprec_amd.embedding.variable import EmbeddingVariable
    with pytest.raises(NotImplementedError, match="HBM_FP8.*CUDA"):
        EmbeddingVariable("e", 8, ev_option=_fp8_option(), device="cpu")
    with pytest.raises(NotImplementedError, match="HBM_FP8.*CUDA"):
        EmbeddingCollection("c", ["a", "b"], 8, ev_option=_fp8_option(),
                            device="cpu")


def test_converter_rejects_cpu_and_unsupported_kinds():
    from deeprec_amd.embedding.collection import EmbeddingCollection
    from deeprec_amd.embedding.extras import MultiHashVariable
    from deeprec_amd.embedding.variable import EmbeddingVariable
    from deeprec_amd.ops.fp8 import quantize_embeddings_fp8
    ev = EmbeddingVariable("e", 8, device="cpu")
    with pytest.raises(NotImplementedError, match="CpuStorage"):
        quantize_embeddings_fp8(ev)
    coll = EmbeddingCollection("c", ["a", "b"], 8, device="cpu")
    with pytest.raises(NotImplementedError, match="CpuStorage"):
        quantize_embeddings_fp8(coll)

    class Model:
        def embedding_variables(self):
            return [ev]
    with pytest.raises(NotImplementedError, match="CpuStorage"):
        quantize_embeddings_fp8(Model())
    with pytest.raises(NotImplementedError, match="MultiHashVariable"):
        quantize_embeddings_fp8(object.__new__(MultiHashVariable))
    # nothing was touched
    assert ev.trainable and type(ev.storage).__name__ == "CpuStorage"


def test_load_quantized_raw_round_trips_the_tools_file(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from deeprec_amd.ops.fp8 import dequantize_fp8_rows, quantize_fp8_rows
    from tools.quantize_embeddings import (load_quantized,
                                           load_quantized_raw)
    from tools.quantize_embeddings import main as tool_main
    gen = torch.Generator().manual_seed(3)
    n, dim = 37, 16
    values = torch.randn(n, dim, generator=gen)
    values[5] = 0.0
    ck = tmp_path / "ckpt-1"
    ck.mkdir()
    fn = ck / "ev-t-part0.safetensors"
    save_file({"keys": torch.arange(n) * 7, "values": values,
               "freqs": torch.arange(n), "versions": torch.arange(n) + 2},
              str(fn))
    for fmt in ("fp8", "int8"):      # the tool's own writer, in process
        monkeypatch.setattr(sys, "argv", ["quantize_embeddings.py", str(ck),
                                          "--apply", "--format", fmt])
        tool_main()
    out = str(fn).replace(".safetensors", ".fp8.safetensors")
    keys, q, scale, freqs, versions = load_quantized_raw(out)
    q_ref, s_ref = quantize_fp8_rows(values)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (n, dim)
    assert torch.equal(q, q_ref) and torch.equal(scale, s_ref)
    assert torch.equal(keys, torch.arange(n) * 7)
    assert torch.equal(freqs, torch.arange(n))
    assert torch.equal(versions, torch.arange(n) + 2)
    # the raw triple dequantizes to what load_quantized returns
    _, deq, _, _ = load_quantized(out)
    assert torch.equal(dequantize_fp8_rows(q, scale), deq)
    # int8 stays a file format: it has no resident form
    with pytest.raises(ValueError, match="values_fp8"):
        load_quantized_raw(out.replace(".fp8.", ".int8."))


class _StubStorage:
    """Records what the saver hands a storage."""

    def __init__(self, inference_only):
        if inference_only:
            self.inference_only = True
        self.slabs = {}
        self.calls = []

    def get_slab(self, name, width, init_value, dtype=torch.float32):
        self.slabs[name] = (width, init_value)

    def import_(self, keys, values, freqs=None, versions=None,
                slab_rows=None):
        self.calls.append((keys, values, freqs, versions, slab_rows))


class _StubEv:
    def __init__(self, inference_only):
        self.name = "stub"
        self.device = torch.device("cpu")
        self.storage = _StubStorage(inference_only)


@pytest.mark.parametrize("incremental", [False, True],
                         ids=["full", "incremental"])
def test_saver_keeps_slabs_away_from_an_inference_only_storage(
        tmp_path, incremental):
    from safetensors.torch import save_file
    from deeprec_amd.checkpoint.saver import Saver
    n = 6
    payload = {"keys": torch.arange(n), "values": torch.randn(n, 4),
               "freqs": torch.arange(n), "versions": torch.arange(n),
               "slab/adam_m": torch.ones(n, 4),
               "slab/adam_v": torch.ones(n, 4),
               "slabinit/adam_m": torch.tensor(0.0),
               "slabinit/adam_v": torch.tensor(0.0)}
    save_file(payload, str(tmp_path / "ev-stub-part0.safetensors"))
    for inference_only in (True, False):
        ev = _StubEv(inference_only)
        saver = Saver(embedding_variables=[ev])
        if incremental:
            saver._restore_ev_files(str(tmp_path), replay=True)
        else:
            saver._restore_ev(str(tmp_path), ev)
        (keys, values, freqs, versions, slab_rows), = ev.storage.calls
        assert torch.equal(keys, payload["keys"])
        assert torch.equal(values, payload["values"])
        assert torch.equal(freqs, payload["freqs"])
        assert torch.equal(versions, payload["versions"])
        if inference_only:
            assert ev.storage.slabs == {} and slab_rows is None
            assert values.device.type == "cpu"
        else:
            assert sorted(ev.storage.slabs) == ["adam_m", "adam_v"]
            assert sorted(slab_rows) == ["adam_m", "adam_v"]
