"""vln-goat_amd — MI355X-native (gfx950) implementation of GOAT's cross-modal transformer hot path.

Import as `vln_goat_amd` (the sibling alias package maps the importable name onto this directory).
Contents: csrc/ (HIP kernels + C ABI), _lib.py (ctypes binding), hipops.py (the op namespace: a facade over one module per op family —
rng.py, ops_gemm.py, ops_linear.py, ops_norm.py, ops_attention.py, ops_dict.py, ops_embed.py, ops_heads.py — and over the layers below
them: _plumbing.py, shadows.py, gradsink.py, tuning.py (GEMM autotuner), streams.py, wgrad_queue.py (deferred grouped weight
gradients)), layers.py / pretrain_model.py / nav_model.py (reference-compatible nn.Module trees for pre-training
and navigation fine-tuning), graphmap.py (host index building), dp.py (gradient arena + data-parallel engine over RCCL),
synth.py (synthetic batches / episodes), frontdoor.py (FACL dictionaries: feature TSV, device k-means, cluster pick),
backdoor.py (BACL dictionaries: token pick plan, running means on the device, room-type image dictionary),
evaluate.py (navigation validation: eval_metrics on the device), pretrain_eval.py (pre-training validation: validate / validate_mlm /
_mrc / _sap / _og / _cfp over device-side statistics),
config.py, tuned_gfx950.json (autotuned GEMM table).
"""
from .layers import compute_dtype, set_compute_dtype  # noqa: F401
from .hipops import manual_seed  # noqa: F401
from .frontdoor import (TIM_TSV_FIELDNAMES, DeviceKMeans, KMeansPicker, extract_front_features, read_tim_tsv,  # noqa: F401
                        write_tim_tsv)
from .backdoor import (InstrDictionaries, InstrPickPlan, build_img_zdict, img_zdict_keys, pick_positions,  # noqa: F401
                       write_img_zdict)
from .pretrain_eval import ValStats, validate_cfp, validate_mlm, validate_mrc, validate_og, validate_sap  # noqa: F401

__version__ = '0.1.0'
