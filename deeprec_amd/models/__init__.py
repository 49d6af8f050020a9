import functools

from deeprec_amd.models.dlrm import DLRM  # noqa: F401
from deeprec_amd.models.zoo import (  # noqa: F401
    DBMTL, DCN, DSSM, ESMM, WDL, DeepFM, MMoE, MaskNet,
    MLPerfDLRMDCN, PLE,
    SimpleMultiTask)
from deeprec_amd.models.sequence import BST, DIEN, DIN  # noqa: F401

MODEL_REGISTRY = {
    "dlrm": DLRM, "wdl": WDL, "wide_and_deep": WDL, "deepfm": DeepFM,
    "dcn": DCN, "dssm": DSSM,
    # a partial, not a lambda: the runner reads the constructor's keywords
    "dcnv2": functools.partial(DCN, v2=True),
    "mmoe": MMoE, "esmm": ESMM, "dbmtl": DBMTL, "ple": PLE,
    "masknet": MaskNet, "simple_multitask": SimpleMultiTask,
    "mlperf_dlrm_dcn": MLPerfDLRMDCN,
    "din": DIN, "dien": DIEN, "bst": BST,
}
SEQUENCE_MODELS = {"din", "dien", "bst"}
