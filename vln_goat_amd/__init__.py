"""Importable name of the product package directory `vln-goat_amd/` (a hyphen is not a valid Python identifier): this package's
search path IS that directory, so `vln_goat_amd.hipops`, `vln_goat_amd.rollout`, ... are the modules there; the public
names of its `__init__` are re-exported by plain imports."""
import os as _os

__path__ = [_os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), 'vln-goat_amd')]

from .layers import compute_dtype, set_compute_dtype  # noqa: E402,F401
from .hipops import manual_seed  # noqa: E402,F401
from .frontdoor import (TIM_TSV_FIELDNAMES, DeviceKMeans, KMeansPicker, extract_front_features, read_tim_tsv,  # noqa: E402,F401
                        write_tim_tsv)
from .backdoor import (InstrDictionaries, InstrPickPlan, build_img_zdict, img_zdict_keys, pick_positions,  # noqa: E402,F401
                       write_img_zdict)
from .pretrain_eval import ValStats, validate_cfp, validate_mlm, validate_mrc, validate_og, validate_sap  # noqa: E402,F401

__version__ = '0.1.0'
