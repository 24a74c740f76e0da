"""The back-door dictionary pipeline (csrc/zdict.hip, hipops.dict_*, backdoor.py), the part that needs no GPU: the two entry points
are declared, exported and bound and reject bad arguments before any launch (no kernel runs: every call below fails validation or has
nothing to write), the wrappers are inference-only, and the host half — the token walk, the pick plan, the file formats and the choice of
room-type labels — does what the reference's loops do."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2
NAMES = ('goat_dict_accumulate', 'goat_dict_finish')


def _lib():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _aligned(nbytes=1024):
    buf = (ctypes.c_char * (nbytes + 16))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_dict_entry_points_are_declared_exported_and_bound():
    lib = _lib()
    txt = open(os.path.join(ROOT, 'include', 'goat_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    h = lib.lib()
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert hasattr(h, name) and name in lib.SIGNATURES
    assert h.goat_version() >= 105
    assert 'zdict.hip' in lib.SOURCES


def test_accumulate_and_finish_argument_validation_without_gpu():
    h = _lib().lib()
    keep, p = _aligned()

    def acc(dtype=0, X=p, rows=p, start=p, sum=p, comp=p, count=p, ld=16, R=4, P=3, D=16, K=3):
        return h.goat_dict_accumulate(None, dtype, X, ld, R, rows, start, sum, comp, count, P, D, K)
    for name in ('X', 'rows', 'start', 'sum', 'comp', 'count'):
        assert acc(**{name: None}) == E_ARG, name
    assert acc(dtype=2) == E_ARG
    assert acc(K=0) == E_SHAPE
    assert acc(K=65536) == E_SHAPE
    assert acc(P=0) == E_SHAPE
    assert acc(D=12, ld=12) == E_SHAPE
    assert acc(D=0) == E_SHAPE
    assert acc(ld=8) == E_SHAPE                            # ld_x < D
    assert acc(X=p + 8) == E_SHAPE                         # base not 16-byte aligned
    assert acc(dtype=1, ld=20) == E_SHAPE                  # bf16: 20 elements are not a multiple of the 8-element chunk
    assert acc(R=0) == E_SHAPE
    assert acc(sum=p + 8) == E_SHAPE

    def fin(dtype=0, sum=p, comp=p, count=p, feats=p, out=p, pz=p, B=2, D=16, K=3):
        return h.goat_dict_finish(None, dtype, sum, comp, count, feats, out, pz, B, D, K)
    for name in ('sum', 'comp', 'count'):
        assert fin(**{name: None}) == E_ARG, name
    assert fin(dtype=2) == E_ARG
    assert fin(B=0) == E_SHAPE
    assert fin(K=0) == E_SHAPE
    assert fin(K=65536) == E_SHAPE
    assert fin(D=12) == E_SHAPE
    assert fin(out=p + 8) == E_SHAPE
    assert fin(feats=None, out=None, pz=None) == 0         # valid, and nothing to launch
    del keep


def test_dict_wrappers_refuse_cpu_tensors_and_grad():
    from vln_goat_amd import hipops
    assert hipops.DICT_PIECE == 64
    x = torch.zeros(4, 16)
    rows, start = torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    state = hipops.DictState(3, 16, 'cpu')
    assert tuple(state.sum.shape) == tuple(state.comp.shape) == (3, 16) and state.count.dtype == torch.int32
    assert state.zero() is state
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.dict_accumulate(x, rows, start, state)
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.dict_accumulate(x.clone().requires_grad_(), rows, start, state)
    with pytest.raises(RuntimeError, match='GPU'):
        hipops.dict_finish(state, feats=torch.zeros(3, 16))
    with pytest.raises(RuntimeError, match='inference-only'):
        hipops.dict_finish(state, out=torch.zeros(2, 3, 16).requires_grad_())
    with pytest.raises(ValueError):
        hipops.DictState(0, 16, 'cpu')
    with pytest.raises(ValueError):
        hipops.DictState(65536, 16, 'cpu')
    with pytest.raises(ValueError):
        hipops.DictState(3, 12, 'cpu')


def test_backdoor_is_exported():
    import vln_goat_amd
    from vln_goat_amd import backdoor
    for name in ('pick_positions', 'InstrPickPlan', 'InstrDictionaries', 'build_img_zdict', 'img_zdict_keys', 'write_img_zdict'):
        assert getattr(vln_goat_amd, name) is getattr(backdoor, name)


# ----------------------------------------------------------------------------- the token walk
def test_pick_positions_hand_written_cases():
    from vln_goat_amd.backdoor import pick_positions
    #          word 0   word 1          word 2    word 3         word 4
    tokens = ['walk', 'past', '##ing', 'the', 'fire', '##place', 'left']
    # a continuation token between two picked words: 'past(##ing)' is word 1 at token 1, 'the' is word 2 at token 3
    assert pick_positions(tokens, [(1, 'past'), (2, 'the')], []) == [(2, 'landmark', 'past'), (4, 'landmark', 'the')]
    # the word count skips both continuation pieces: word 4 is token 6
    assert pick_positions(tokens, [(3, 'fireplace')], [(4, 'left')]) == [(5, 'landmark', 'fireplace'), (7, 'direction', 'left')]
    # a landmark and a direction on one word: both fire, landmark first
    assert pick_positions(tokens, [(0, 'walk')], [(0, 'go')]) == [(1, 'landmark', 'walk'), (1, 'direction', 'go')]
    # picks beyond the token list are never reached
    assert pick_positions(tokens, [(4, 'left'), (5, 'nothing')], [(9, 'far')]) == [(7, 'landmark', 'left')]
    # an entry that is never reached blocks the entries behind it (the reference only ever looks at the next unused entry)
    assert pick_positions(tokens, [(2, 'the'), (1, 'past'), (3, 'fireplace')], []) == [(4, 'landmark', 'the')]
    assert pick_positions(tokens, [], []) == []
    assert pick_positions([], [(0, 'a')], [(0, 'b')]) == []


# ----------------------------------------------------------------------------- the plan
def _five():
    """5 instructions; tokens are one per word except item 2, whose second word has a continuation piece.  ids: [CLS]=1, word ids, [SEP]=2."""
    data = []
    spec = [
        (['go', 'left', 'door'], [(2, 'door')], [(1, 'left')]),
        (['turn', 'right', 'at', 'the', 'table'], [(4, 'table')], [(0, 'turn'), (1, 'right')]),
        (['walk', 'up', '##stairs', 'door'], [(2, 'door')], [(1, 'up')]),
        (['stop'], [], []),
        (['left', 'table', 'left', 'chair'], [(1, 'table'), (3, 'chair')], [(0, 'left'), (2, 'left')]),
    ]
    for i, (toks, lm, di) in enumerate(spec):
        data.append({'instr_id': 'i%d' % i, 'instruction': ' '.join(toks), 'instr_encoding': [1] + list(range(10, 10 + len(toks))) + [2],
                     'tokens': toks, 'landmarks': lm, 'directions': di})
    return data


def _plan(data, **kw):
    from vln_goat_amd.backdoor import InstrPickPlan
    return InstrPickPlan(data, lambda it: it['tokens'], lambda it: (it['landmarks'], it['directions']), **kw)


def test_pick_plan_slots_counts_and_batches():
    plan = _plan(_five(), batch_size=2)
    assert plan.keys == {'landmark': ['door', 'table', 'chair'], 'direction': ['left', 'turn', 'right', 'up']}
    assert plan.counts == {'landmark': {'door': 2, 'table': 2, 'chair': 1}, 'direction': {'left': 3, 'turn': 1, 'right': 1, 'up': 1}}
    assert plan.pz == {'landmark': {'door': 2 / 5, 'table': 2 / 5, 'chair': 1 / 5},
                       'direction': {'left': 3 / 6, 'turn': 1 / 6, 'right': 1 / 6, 'up': 1 / 6}}
    assert [b.size for b in plan.batches] == [2, 2, 1]
    assert [tuple(b.ids.shape) for b in plan.batches] == [(2, 7), (2, 6), (1, 6)]
    b0 = plan.batches[0]
    assert b0.ids.dtype == torch.int64 and b0.mask.dtype == torch.bool and b0.picks.dtype == torch.int32
    assert b0.ids.tolist() == [[1, 10, 11, 12, 2, 0, 0], [1, 10, 11, 12, 13, 14, 2]]
    assert b0.mask.tolist() == [[True] * 5 + [False] * 2, [True] * 7]
    # rows are b * Lmax + pos, grouped by slot; start has one entry per slot of the WHOLE pass
    assert b0.rows('landmark').tolist() == [3, 7 + 5] and b0.start('landmark', 3).tolist() == [0, 1, 2, 2]
    assert b0.rows('direction').tolist() == [2, 7 + 1, 7 + 2] and b0.start('direction', 4).tolist() == [0, 1, 2, 3, 3]
    b1 = plan.batches[1]                                  # item 2: 'door' is token 3 -> pos 4 (the continuation piece shifts it); item 3 picks nothing
    assert b1.rows('landmark').tolist() == [4] and b1.start('landmark', 3).tolist() == [0, 1, 1, 1]
    assert b1.rows('direction').tolist() == [2] and b1.start('direction', 4).tolist() == [0, 0, 0, 0, 1]
    b2 = plan.batches[2]                                  # 'left' twice in one instruction: two rows in one slot
    assert b2.rows('landmark').tolist() == [2, 4] and b2.start('landmark', 3).tolist() == [0, 0, 1, 2]
    assert b2.rows('direction').tolist() == [1, 3] and b2.start('direction', 4).tolist() == [0, 2, 2, 2, 2]
    assert b2.max_rows == {'landmark': 1, 'direction': 2}
    for b in plan.batches:                                # consistency: every start ends at the number of rows, slots ascend
        for kind, K in (('landmark', 3), ('direction', 4)):
            start = b.start(kind, K).tolist()
            assert start[0] == 0 and start[-1] == len(b.rows(kind)) and start == sorted(start)
            assert all(0 < r < b.ids.numel() for r in b.rows(kind).tolist())


def test_pick_plan_without_picks_in_a_batch_and_landmark_only():
    data = _five()
    plan = _plan(data[3:4] + data[:1], batch_size=1)
    assert plan.batches[0].layout == {} and plan.batches[0].picks.numel() == 0
    assert sorted(plan.batches[1].layout) == ['direction', 'landmark']
    only = _plan(data, batch_size=2, kinds=('landmark',))
    assert only.keys == {'landmark': ['door', 'table', 'chair'], 'direction': []} and only.pz['direction'] == {}
    assert all(list(b.layout) in ([], ['landmark']) for b in only.batches)


def test_pick_plan_refuses_a_pick_beyond_the_instruction():
    data = _five()
    data[1]['instr_encoding'] = data[1]['instr_encoding'][:4]          # 'table' is pos 5 of an encoding of 4
    with pytest.raises(ValueError, match='picks token row 5'):
        _plan(data, batch_size=2)
    with pytest.raises(ValueError, match='picks token row'):
        _plan(_five(), batch_size=2, max_len=4)


# ----------------------------------------------------------------------------- files
def test_save_tsv_round_trip_with_stubbed_features(tmp_path):
    from vln_goat_amd import features
    from vln_goat_amd.backdoor import InstrDictionaries
    rs = np.random.RandomState(3)
    d = InstrDictionaries('cpu', H=16)
    d.feats = {'landmark': torch.from_numpy(rs.standard_normal((3, 16)).astype(np.float32)),
               'direction': torch.from_numpy(rs.standard_normal((2, 16)).astype(np.float32))}
    d.keys = {'landmark': ['door', 'table', 'chair'], 'direction': ['left', 'turn']}
    d.host_pz = {'landmark': {'door': 2 / 5, 'table': 2 / 5, 'chair': 1 / 5}, 'direction': {'left': 1 / 3, 'turn': 2 / 3}}
    path = str(tmp_path / 'backdoor_update_features.tsv')
    d.save_tsv(path)
    lines = [l.split('\t') for l in open(path).read().splitlines()]
    assert [(l[0], l[1]) for l in lines] == [('landmark', 'door'), ('landmark', 'table'), ('landmark', 'chair'), ('direction', 'left'),
                                             ('direction', 'turn')]
    z = features.load_instr_zdict(path)
    assert torch.equal(z['instr_landmark_features'], d.feats['landmark']) and torch.equal(z['instr_direction_features'], d.feats['direction'])
    assert z['instr_landmark_pzs'].tolist() == [2 / 5, 2 / 5, 1 / 5] and z['instr_direction_pzs'].tolist() == [1 / 3, 2 / 3]
    again = InstrDictionaries('cpu', H=16).load_tsv(path)
    assert again.keys == d.keys and again.host_pz == d.host_pz
    assert torch.equal(again.feats['landmark'], d.feats['landmark']) and again.pzs['direction'].dtype == torch.float32
    zd = again.z_dict()['instr_zdict']
    assert sorted(zd) == ['instr_direction_features', 'instr_direction_pzs', 'instr_landmark_features', 'instr_landmark_pzs']
    with pytest.raises(ValueError, match='kinds'):
        InstrDictionaries('cpu', kinds=('object',))


def test_img_zdict_keys_ties_order_and_pz(tmp_path):
    from vln_goat_amd import features
    from vln_goat_amd.backdoor import img_zdict_keys, write_img_zdict
    # counts: hall 3, kitchen 2, bath 2, stairs 2, porch 1.  roomnum = 3 cuts inside the tie at 2: the stable sort keeps the labels that
    # were SEEN first (kitchen at s_a, bath at s_a), stairs (first seen at s_b) falls out.  Rows: first appearance among the kept.
    table = {'s_a': ['kitchen', 'hall', 'bath'], 's_b': ['stairs', 'hall', 'kitchen'], 's_c': ['porch', 'bath', 'stairs'], 's_d': ['hall']}
    order, counts, pz = img_zdict_keys(table, roomnum=3)
    assert order == ['kitchen', 'hall', 'bath']
    assert counts == {'kitchen': 2, 'hall': 3, 'bath': 2}
    assert pz == {'kitchen': 2 / 7, 'hall': 3 / 7, 'bath': 2 / 7}
    order, counts, pz = img_zdict_keys(table, roomnum=50)
    assert order == ['kitchen', 'hall', 'bath', 'stairs', 'porch'] and sum(counts.values()) == 10 and pz['porch'] == 1 / 10
    assert img_zdict_keys(table, roomnum=1) == (['hall'], {'hall': 3}, {'hall': 1.0})
    assert img_zdict_keys({}, roomnum=3) == ([], {}, {})
    rs = np.random.RandomState(4)
    z = {'img_features': torch.from_numpy(rs.standard_normal((3, 8)).astype(np.float32)),
         'img_pzs': torch.tensor([2 / 7, 3 / 7, 2 / 7], dtype=torch.float64), 'roomtypes': ['kitchen', 'hall', 'bath']}
    path = str(tmp_path / 'image_z_dict_3.tsv')
    write_img_zdict(path, z)
    back = features.load_img_zdict(path)
    assert torch.equal(back['img_features'], z['img_features']) and torch.equal(back['img_pzs'], z['img_pzs'])
    assert [l.split('\t')[0] for l in open(path).read().splitlines()] == z['roomtypes']
