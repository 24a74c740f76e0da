"""The op namespace of the package: every hand-written gfx950 op as `hipops.NAME`.  This file defines nothing; it re-exports.

Every op launches kernels of libgoat_hip.so on the *current torch HIP stream* through ctypes (`_lib.py`); nothing synchronises or
allocates outside torch's caching allocator, so a whole forward+backward step can be captured into a hipGraph (`torch.cuda.graph`).
There is no eager/CPU fallback: CPU tensors raise.  Compute dtype: float32 (exact-f32 MFMA, the 1e-3 parity mode) or bfloat16 (bf16
storage, f32 accumulate).  Parameters stay float32 masters; bf16 / transposed "shadows" of the weights are cached on the Parameter
object and refreshed when its version counter moves (i.e. once per optimizer step).

Where things live (each module imports downward only; none imports this one):
  rng            RngState, manual_seed: the dropout counter
  ops_gemm       gemm_nt, transpose_pad, colsum, gemm (autotuner / profile hooks, split-K rules), wgrad, linear_wgrad; loads the tuned table
  ops_linear     linear (Linear, RowDot), act_bwd, ffn, decoder_cross_entropy, multi_linear, linear_bank
  ops_norm       layer_norm, dropout_add, dropout, add_n, fanout, fanout_tree, zero_ranges
  ops_attention  attention; DecodeState, attn_decode, decode_select (KV-cached decoding, inference only)
  ops_dict       kmeans_*; DictState, dict_accumulate, dict_finish (inference only)
  ops_embed      embedding (+ SparseEmbedGrad, check_embed_errors), pano_fusion, gather_segmean
  ops_heads      cross_entropy_rows, attn_pool, door_gate, dict_weighted_sum, sap_fuse, infonce, cfp_mix, cfp_tail, backward_mean;
                 val_rows, val_cfp, val_reduce (validation statistics, inference only)
  ops_text       retok_rows (+ check_retok_status), scale_cols (back-translation: words to instruction rows, shared feature mask;
                 inference only)
and below them: _plumbing (pointers, launch), shadows (weight copies), gradsink (arena slices), tuning (GEMM configurations, AUTOTUNE,
PROFILE), streams (graph capture, branches), wgrad_queue (deferred weight gradients and LayerNorm reductions).

Switches that are read at call time (`hipops.AUTOTUNE`, `hipops.LN_DETERMINISTIC`, ...) are not copied here: reading or writing them
through this module reads or writes the global of their home module (_HipopsModule._FORWARD).
"""
import sys as _sys

import torch                                                            # noqa: F401

from . import _lib, ops_embed, ops_linear, ops_norm, tuning             # noqa: F401
from ._lib import GOAT_BF16, GOAT_F32, EPI_ACCUM, EPI_GELU, EPI_MUL_DGELU, EPI_MUL_DRELU, EPI_NONE, EPI_RELU      # noqa: F401
from ._plumbing import _dt, _epc, _inference_only, _need_gpu, _ptr, _rows, _stream, call, cargs, launch      # noqa: F401
from .shadows import _bias_padded, _cat_bias, _shadow, _shadow_cat, _shadow_rows_padded, _store_shadow, refresh_shadows      # noqa: F401
from .gradsink import ARENA_EPOCH, _first_touch, _prep_fallback, _sink, _sink_cat, small_sinks      # noqa: F401
from .tuning import (BALANCED, EIGHT_WAVES, PERSIST, PINGPONG, TUNED_FILE, TUNE_EVENTS, USE_PERSIST, USE_PP, _FLUSH, _TUNED,      # noqa: F401
                     _heuristic_cfg, _launch_gemm_bf16, _tile_candidates, _time_cfg, _tune_gemm, load_tuned, n_cu, save_tuned, stage_name, tile, tile_name)
from .streams import Branch, graph, note_parallel_branch, _RETAINED_GRAPHS          # noqa: F401
from .wgrad_queue import LnReduceQueue, WgradQueue                                   # noqa: F401
from .rng import RngState, manual_seed                                               # noqa: F401
from .ops_gemm import _profile_start, _split_k, colsum, gemm, gemm_nt, linear_wgrad, transpose_pad, wgrad      # noqa: F401
from .ops_linear import (_ACT_DEPI, _ACT_EPI, _DecoderCeFn, _FfnFn, _GradSlots, _LinearBankFn, _LinearFn, _MultiLinearFn, _RowDotFn,      # noqa: F401
                         _pad_k, act_bwd, decoder_cross_entropy, ffn, linear, linear_bank, multi_linear)
from .ops_norm import _DropAddFn, _FanoutFn, _LnFn, add_n, dropout, dropout_add, fanout, fanout_tree, layer_norm, zero_ranges      # noqa: F401
from .ops_attention import (ATTN_MAXLK, ATTN_SHORT_MAXLK, DECODE_MAXL, DecodeState, _AttnFn, _attn_entry, _attn_layout, attention,      # noqa: F401
                            attn_decode, decode_select)
from .ops_dict import (DICT_MAXK, DICT_PIECE, KMEANS_MAXK, DictState, _dict_state, _kmeans_i32, _kmeans_x, dict_accumulate, dict_finish,      # noqa: F401
                       kmeans_assign, kmeans_centres, kmeans_csr, kmeans_pick)
from .ops_embed import (_EMBED_ERR, SparseEmbedGrad, _EmbedFn, _GatherFn, _PanoFusionFn, _embed_err, check_embed_errors, embedding,      # noqa: F401
                        embedding_scatter_add, gather_segmean, pano_fusion)
from .ops_heads import (_MEAN_SEED, _AttnPoolFn, _CeRowsFn, _CfpMixFn, _CfpTailFn, _DictWsumFn, _DoorGateFn, _InfoNceFn, _SapFuseFn,      # noqa: F401
                        _cfp_mix_bwd, _cfp_mix_fwd, _u8, attn_pool, backward_mean, cfp_mix, cfp_tail, cross_entropy_rows, dict_weighted_sum,
                        door_gate, infonce, sap_fuse, val_cfp, val_reduce, val_rows)
from .ops_text import RETOK_MAXB, RETOK_MAXL, RETOK_STATUS, check_retok_status, retok_rows, scale_cols      # noqa: F401


class _HipopsModule(type(_sys)):
    """Module-level state that is read at call time lives in one place, the module that reads it: `hipops.NAME` for a name in _FORWARD
    reads and writes that module's global (bench.py, the tests and scripts switch AUTOTUNE, PROFILE and the A/B flags through hipops).
    A forwarded name must not be bound in this module's own dictionary, or __getattr__ is never asked."""
    _FORWARD = {'AUTOTUNE': tuning, 'PROFILE': tuning,
                'ROWDOT': ops_linear, 'SMALLK_WGRAD': ops_linear, 'LINEAR_BANK': ops_linear,
                'LN_DETERMINISTIC': ops_norm, 'LN_ATOMIC_MAX_ROWS': ops_norm, 'FANOUT': ops_norm,
                'PANO_SINK': ops_embed}

    def __getattr__(self, name):
        home = _HipopsModule._FORWARD.get(name)
        if home is not None:
            return getattr(home, name)
        raise AttributeError('module %r has no attribute %r' % (self.__name__, name))

    def __setattr__(self, name, value):
        home = _HipopsModule._FORWARD.get(name)
        if home is not None:
            setattr(home, name, value)
        else:
            super().__setattr__(name, value)

    def __dir__(self):
        return sorted(set(super().__dir__()) | set(_HipopsModule._FORWARD))


_sys.modules[__name__].__class__ = _HipopsModule
