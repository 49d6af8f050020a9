"""Values and types shared by the engine wrappers (ops) and the embedding
layer. Imports nothing from the package, so either side can use it
without a cycle."""
import math
from typing import NamedTuple, Optional

import torch

COMBINER_ID = {"sum": 0, "mean": 1, "sqrtn": 2}
KEY_BITS = 48              # composite key = table_id << KEY_BITS | raw id
PAD_KEY = (1 << 63) - 1    # == ext.PAD_KEY, the padded exchange's wire pad


class Slab(NamedTuple):
    """One state slab of a sparse optimizer, a row per value slot."""
    name: str                # checkpoints store the slab under this name
    width: Optional[int]     # None: as wide as the values (storage.dim)
    init_key: Optional[str]  # hyper key that overrides the initial value
    init: float              # initial value of every row


_ACCUM = Slab("adagrad_accum", None, "initial_accumulator", 0.1)
_ADAM_M = Slab("adam_m", None, None, 0.0)
_ADAM_V = Slab("adam_v", None, None, 0.0)

# The state of every sparse apply rule, in the order the HIP entry point
# takes the slabs. The keys are the sparse optimizer names, plus the two
# other forms adam_async takes: "rmsprop" (sparse_rmsprop: no first
# moment) and "adam_dev" (beta powers on the device, HIP only).
OPTIMIZER_SLABS = {
    "sgd": (),
    "adagrad": (_ACCUM,),
    "adagrad_decay": (_ACCUM, Slab("adagrad_decay_period", 1, None, 0.0)),
    "adam": (_ADAM_M, _ADAM_V),
    "adamw": (_ADAM_M, _ADAM_V),
    "adam_async": (_ADAM_M, _ADAM_V),
    "adam_dev": (_ADAM_M, _ADAM_V),
    "rmsprop": (_ADAM_V,),
    "ftrl": (Slab("ftrl_accum", None, None, 0.1),
             Slab("ftrl_linear", None, None, 0.0)),
}
SLAB_NAMES = list(dict.fromkeys(
    s.name for slabs in OPTIMIZER_SLABS.values() for s in slabs))


def optimizer_slabs(storage, rule: str, hyper: dict) -> list:
    """The rule's state slabs of `storage`, created on first use."""
    return [storage.get_slab(s.name, s.width or storage.dim,
                             hyper.get(s.init_key, s.init))
            for s in OPTIMIZER_SLABS[rule]]


def bias_corrected_lr(lr, beta1_power, beta2_power):
    """Adam's step size with both moments' bias corrections folded in."""
    return lr * math.sqrt(1 - beta2_power) / (1 - beta1_power)


class DedupResult(NamedTuple):
    """One step's unique keys and everything derived with them. The
    fields belong together: `rank` only orders the occurrences of THIS
    `inverse`, so it travels with it instead of being looked up later."""
    uniq: torch.Tensor                # unique keys (nnz-padded in capture)
    inverse: torch.Tensor             # i32 occurrence -> unique row
    counts: Optional[torch.Tensor]    # occurrences per unique key
    slots: Optional[torch.Tensor]     # None: requester-side pass, no probe
    rank: Optional[torch.Tensor]      # pass C's rank of each occurrence
    #                                   within its key; None on the sort path
    m_dev: Optional[torch.Tensor]     # device unique count; None when the
    #                                   host knows it (uniq.numel())
