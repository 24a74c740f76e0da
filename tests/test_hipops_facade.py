"""hipops is a facade: every name that was reachable as `hipops.NAME` while the ops lived in that one file still is, functions and
classes are the objects of their home modules, the switches that are read at call time are forwarded to the module that reads them,
and no op-family module imports the facade.  Runs on the CPU: nothing is launched."""
import ast
import importlib
import os

import pytest

# dir(hipops) of the single-file layout, without dunders and the standard-library modules it happened to import, by home module
_HOME = {
    '_lib': ['EPI_ACCUM', 'EPI_GELU', 'EPI_MUL_DGELU', 'EPI_MUL_DRELU', 'EPI_NONE', 'EPI_RELU', 'GOAT_BF16', 'GOAT_F32'],
    '_plumbing': ['_dt', '_epc', '_inference_only', '_need_gpu', '_ptr', '_rows', '_stream', 'call', 'cargs', 'launch'],
    'shadows': ['_bias_padded', '_cat_bias', '_shadow', '_shadow_cat', '_shadow_rows_padded', '_store_shadow', 'refresh_shadows'],
    'gradsink': ['ARENA_EPOCH', '_first_touch', '_prep_fallback', '_sink', '_sink_cat', 'small_sinks'],
    'tuning': ['BALANCED', 'EIGHT_WAVES', 'PERSIST', 'PINGPONG', 'TUNED_FILE', 'TUNE_EVENTS', 'USE_PERSIST', 'USE_PP', '_FLUSH', '_TUNED',
               '_heuristic_cfg', '_launch_gemm_bf16', '_tile_candidates', '_time_cfg', '_tune_gemm', 'load_tuned', 'n_cu', 'save_tuned',
               'stage_name', 'tile', 'tile_name'],
    'streams': ['Branch', '_RETAINED_GRAPHS', 'graph', 'note_parallel_branch'],
    'wgrad_queue': ['LnReduceQueue', 'WgradQueue'],
    'rng': ['RngState', 'manual_seed'],
    'ops_gemm': ['_profile_start', '_split_k', 'colsum', 'gemm', 'gemm_nt', 'linear_wgrad', 'transpose_pad', 'wgrad'],
    'ops_linear': ['LINEAR_BANK', 'ROWDOT', 'SMALLK_WGRAD', '_ACT_DEPI', '_ACT_EPI', '_DecoderCeFn', '_FfnFn', '_GradSlots', '_LinearBankFn',
                   '_LinearFn', '_MultiLinearFn', '_RowDotFn', '_pad_k', 'act_bwd', 'decoder_cross_entropy', 'ffn', 'linear', 'linear_bank',
                   'multi_linear'],
    'ops_norm': ['FANOUT', 'LN_ATOMIC_MAX_ROWS', 'LN_DETERMINISTIC', '_DropAddFn', '_FanoutFn', '_LnFn', 'add_n', 'dropout', 'dropout_add',
                 'fanout', 'fanout_tree', 'layer_norm', 'zero_ranges'],
    'ops_attention': ['ATTN_MAXLK', 'ATTN_SHORT_MAXLK', 'DECODE_MAXL', 'DecodeState', '_AttnFn', '_attn_entry', '_attn_layout', 'attention',
                      'attn_decode', 'decode_select'],
    'ops_dict': ['DICT_MAXK', 'DICT_PIECE', 'DictState', 'KMEANS_MAXK', '_dict_state', '_kmeans_i32', '_kmeans_x', 'dict_accumulate',
                 'dict_finish', 'kmeans_assign', 'kmeans_centres', 'kmeans_csr', 'kmeans_pick'],
    'ops_embed': ['PANO_SINK', 'SparseEmbedGrad', '_EMBED_ERR', '_EmbedFn', '_GatherFn', '_PanoFusionFn', '_embed_err', 'check_embed_errors',
                  'embedding', 'embedding_scatter_add', 'gather_segmean', 'pano_fusion'],
    'ops_heads': ['_AttnPoolFn', '_CeRowsFn', '_CfpMixFn', '_CfpTailFn', '_DictWsumFn', '_DoorGateFn', '_InfoNceFn', '_MEAN_SEED', '_SapFuseFn',
                  '_cfp_mix_bwd', '_cfp_mix_fwd', '_u8', 'attn_pool', 'backward_mean', 'cfp_mix', 'cfp_tail', 'cross_entropy_rows',
                  'dict_weighted_sum', 'door_gate', 'infonce', 'sap_fuse'],
}
_OWN = ['_HipopsModule', '_lib', 'torch', 'tuning']          # the forwarder class and the modules that are reachable through hipops

# name -> home module of the state that is read at call time (a copy in hipops would make a write through hipops a silent no-op)
_FORWARDED = {'AUTOTUNE': 'tuning', 'PROFILE': 'tuning', 'ROWDOT': 'ops_linear', 'SMALLK_WGRAD': 'ops_linear', 'LINEAR_BANK': 'ops_linear',
              'LN_DETERMINISTIC': 'ops_norm', 'LN_ATOMIC_MAX_ROWS': 'ops_norm', 'FANOUT': 'ops_norm', 'PANO_SINK': 'ops_embed'}

_FAMILIES = ['rng', 'ops_gemm', 'ops_linear', 'ops_norm', 'ops_attention', 'ops_dict', 'ops_embed', 'ops_heads']


def _home(module):
    return importlib.import_module('vln_goat_amd.' + module)


def test_the_name_list_is_the_single_file_layouts():
    names = [n for ns in _HOME.values() for n in ns] + _OWN
    assert len(names) == len(set(names)) == 160 and sum(not n.startswith('_') for n in names) == 95
    assert set(_FORWARDED) - {'AUTOTUNE', 'PROFILE'} <= set(names)       # (the two were forwarded before: never in dir())


@pytest.mark.parametrize('module', sorted(_HOME))
def test_every_name_resolves_to_the_object_of_its_home_module(module):
    from vln_goat_amd import hipops
    home = _home(module)
    for name in _HOME[module]:
        obj = getattr(hipops, name)
        if isinstance(obj, (bool, int, str)):
            assert obj == getattr(home, name) and type(obj) is type(getattr(home, name)), name
        else:
            assert obj is getattr(home, name), name
        if isinstance(obj, type) or callable(obj):
            assert obj.__module__ == 'vln_goat_amd.' + module, name


def test_modules_and_the_forwarder_are_reachable():
    import torch
    from vln_goat_amd import _lib, hipops, tuning
    assert hipops._lib is _lib and hipops.tuning is tuning and hipops.torch is torch
    assert type(hipops) is hipops._HipopsModule and set(hipops._HipopsModule._FORWARD) == set(_FORWARDED)
    for name, module in _FORWARDED.items():
        assert hipops._HipopsModule._FORWARD[name] is _home(module), name


@pytest.mark.parametrize('name', sorted(_FORWARDED))
def test_a_forwarded_flag_is_the_global_its_home_module_reads(name, monkeypatch):
    from vln_goat_amd import hipops
    home = _home(_FORWARDED[name])
    assert name not in vars(hipops) and name in vars(home)
    before = getattr(home, name)
    assert getattr(hipops, name) is before
    new = object()
    setattr(hipops, name, new)                      # a plain write, as bench.py switches AUTOTUNE
    try:
        assert vars(home)[name] is new and getattr(hipops, name) is new and name not in vars(hipops)
    finally:
        setattr(hipops, name, before)
    assert vars(home)[name] is before
    other = object()
    with monkeypatch.context() as m:                # the way tests switch LN_DETERMINISTIC
        m.setattr(hipops, name, other)
        assert vars(home)[name] is other and name not in vars(hipops)
    assert vars(home)[name] is before and getattr(hipops, name) is before and name not in vars(hipops)


def test_a_flag_is_read_from_the_module_global_at_call_time():
    """the ops look their switches up as globals of their own module when they run, which is the dictionary hipops writes into"""
    from vln_goat_amd import ops_embed, ops_linear, ops_norm
    for fn, name in ((ops_norm.fanout, 'FANOUT'), (ops_norm._LnFn.backward, 'LN_DETERMINISTIC'), (ops_norm._LnFn.backward, 'LN_ATOMIC_MAX_ROWS'),
                     (ops_linear.linear, 'ROWDOT'), (ops_linear._LinearFn.backward, 'SMALLK_WGRAD'), (ops_embed._PanoFusionFn.backward, 'PANO_SINK')):
        assert fn.__globals__ is vars(importlib.import_module(fn.__module__)) and name in fn.__code__.co_names, name


def test_an_unknown_name_still_raises():
    from vln_goat_amd import hipops
    with pytest.raises(AttributeError):
        hipops.no_such_op
    hipops._facade_probe = 1                        # an ordinary attribute still lands in the facade's own dictionary
    try:
        assert vars(hipops)['_facade_probe'] == 1
    finally:
        del hipops._facade_probe


@pytest.mark.parametrize('module', _FAMILIES)
def test_no_family_module_imports_the_facade(module):
    """by the source text: neither `hipops` as an imported module or name, nor an attribute access on it"""
    home = _home(module)
    tree = ast.parse(open(home.__file__).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            assert not any(a.name.split('.')[-1] == 'hipops' for a in node.names), (module, node.lineno)
        elif isinstance(node, ast.ImportFrom):
            assert (node.module or '').split('.')[-1] != 'hipops' and not any(a.name == 'hipops' for a in node.names), (module, node.lineno)
        elif isinstance(node, ast.Name):
            assert node.id != 'hipops', (module, node.lineno)
    assert 'hipops' not in vars(home)
    assert len(open(home.__file__).read().splitlines()) <= 450, module
    assert os.path.basename(home.__file__) == module + '.py'


def test_rng_draw_consumes_the_counter_as_next_does():
    from vln_goat_amd.rng import RngState
    saved = (RngState.seed, RngState.counter, RngState.dev)
    try:
        RngState.seed, RngState.counter, RngState.dev = 1234, 0, None
        sizes = [1, 7, 8, 9, 16, 1000, 3 * 5 * 7, 0]
        want = []
        for i, n in enumerate(sizes):               # the reference sequence: interleaved next() calls, skipping where p <= 0
            want.append(RngState.next(n) if i % 3 else None)
        end = RngState.counter
        RngState.counter = 0
        for i, n in enumerate(sizes):
            at = RngState.counter
            if i % 3:
                got = RngState.draw(0.1 if i % 2 else 1.0, n)
                assert got == want[i] and got == (1234, at, None)
                assert RngState.counter - at == (n + 7) // 8 * 8 and RngState.counter % 8 == 0
            else:
                assert RngState.draw(0.0, n) == (0, 0, None) and RngState.draw(-1.0, n) == (0, 0, None)
                assert RngState.counter == at       # nothing consumed
        assert RngState.counter == end
    finally:
        RngState.seed, RngState.counter, RngState.dev = saved
