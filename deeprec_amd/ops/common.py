"""Values and types shared by the engine wrappers (ops) and the embedding
layer. Imports nothing from the package, so either side can use it
without a cycle."""
from typing import NamedTuple, Optional

import torch

COMBINER_ID = {"sum": 0, "mean": 1, "sqrtn": 2}
KEY_BITS = 48              # composite key = table_id << KEY_BITS | raw id
PAD_KEY = (1 << 63) - 1    # == ext.PAD_KEY, the padded exchange's wire pad


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
