"""The back-door dictionary kernels (csrc/zdict.hip) and backdoor.py on the GPU.

The bound on a mean comes from the arithmetic contract, not from a measurement: inside a launch a slot's rows are summed in float32 in
pieces of at most DICT_PIECE = 64 rows (a piece of n rows errs by at most (n - 1) u sum|x|, u = 2^-24), every piece sum is folded into
the running pair with a compensated step (about 2 u sum|x| in all, however many launches), the final division adds u.  So per (slot,
column)  |feats - mean64| <= (m + 4) 2^-24 mean64(|x|)  with m = min(64, the most rows one launch gave that slot), the means taken in
float64 over the exact input values (the bf16 values for a bf16 table).  A plain float32 running sum over 300 launches of 1-3
uniform(0, 1) rows misses that bound by 2x, over 2000 launches of one row by 6x (float32 numpy emulation), so those two cases show that
the compensation is there."""
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int32), dtype=torch.int32, device=DEV)


def csr(groups):
    """[[row, ...] per slot] -> (rows int32 [P], start int32 [K+1]) on the device."""
    start = np.zeros(len(groups) + 1, dtype=np.int64)
    start[1:] = np.cumsum([len(g) for g in groups])
    return i32([r for g in groups for r in g]), i32(start)


def check_means(feats, x, launches, counts=None):
    """feats float32 [K, D] against float64 means of the rows of x (device table, its own values) that `launches` ([[rows per slot]]
    per launch, out-of-range rows skipped) gave every slot, within the bound of the module docstring; counts exact."""
    xd = x.detach().double().cpu().numpy()
    R, K = xd.shape[0], len(launches[0])
    got = feats.double().cpu().numpy()
    worst = 0.0
    for k in range(K):
        per_launch = [[r for r in groups[k] if 0 <= r < R] for groups in launches]
        used = [r for g in per_launch for r in g]
        if counts is not None:
            assert int(counts[k]) == len(used), (k, int(counts[k]), len(used))
        if not used:
            assert not got[k].any()
            continue
        m = min(64, max(len(g) for g in per_launch))
        mean, mean_abs = xd[used].mean(0), np.abs(xd[used]).mean(0)
        bound = (m + 4) * U * mean_abs
        err = np.abs(got[k] - mean)
        assert (err <= bound).all(), (k, m, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def run(x, launches):
    from vln_goat_amd import hipops
    state = hipops.DictState(len(launches[0]), x.shape[1], DEV)
    for groups in launches:
        rows, start = csr(groups)
        hipops.dict_accumulate(x, rows, start, state)
    feats = torch.empty(state.K, state.D, device=DEV)
    hipops.dict_finish(state, feats=feats)
    return state, feats


def random_groups(rs, R, K, P):
    """P picks spread over K slots at random (some slots may stay empty when P < K)."""
    slot = rs.randint(0, K, P)
    rows = rs.randint(0, R, P)
    return [[int(r) for r in rows[slot == k]] for k in range(K)]


# ----------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('R,D,K,P', [(97, 768, 3, 41), (64, 16, 1, 1), (515, 40, 300, 1200), (200, 768, 50, 200)])
def test_accumulate_matches_float64_means(R, D, K, P, dtype):
    rs = np.random.RandomState(R + K)
    x = torch.from_numpy(rs.standard_normal((R, D)).astype(np.float32)).to(DEV).to(dtype)
    groups = random_groups(rs, R, K, P)
    state, feats = run(x, [groups])
    check_means(feats, x, [groups], state.count.cpu())
    assert int(state.count.sum()) == P                   # (K = 300: the 256-cluster cap of the k-means kernels does not apply here)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_accumulate_strided_view_empty_slot_repeats_and_out_of_range_rows(dtype):
    rs = np.random.RandomState(7)
    R, D = 60, 40
    full = torch.from_numpy(rs.uniform(-1, 1, (R, D + 8)).astype(np.float32)).to(DEV).to(dtype)
    x = full[:, :D]                                      # ld_x = D + 8
    assert x.stride(0) == D + 8 and not x.is_contiguous()
    groups = [[5, 17, 5, 5, 40],                         # a row repeated inside a slot: it counts every time
              [],                                        # a slot without rows
              [-1, 3, R, 59],                            # two out-of-range rows: neither added nor counted
              [R + 1000, -7]]                            # nothing valid at all
    state, feats = run(x, [groups])
    assert state.count.tolist() == [5, 0, 2, 0]
    check_means(feats, x, [groups], state.count.cpu())
    assert not feats[1].any() and not feats[3].any()
    assert not state.sum[1].any() and not state.comp[1].any()
    # the columns beyond D were never read into the sums
    ref0 = x[[5, 17, 5, 5, 40]].double().mean(0)
    assert torch.allclose(feats[0].double(), ref0, rtol=0, atol=1e-5)


# ----------------------------------------------------------------------------- the running state
@pytest.mark.parametrize('n_launch,max_rows', [(300, 3), (2000, 1)])
def test_running_state_stays_within_the_bound_over_many_launches(n_launch, max_rows):
    from vln_goat_amd import hipops
    rs = np.random.RandomState(n_launch)
    R, D, K = 4096, 16, 2
    x = torch.from_numpy(rs.uniform(0, 1, (R, D)).astype(np.float32)).to(DEV)
    launches = [[[int(r) for r in rs.randint(0, R, rs.randint(1, max_rows + 1))] for _ in range(K)] for _ in range(n_launch)]
    # one upload for all launches: rows and start of launch i are slices of two flat tensors
    flat_rows, flat_start, offs = [], [], [0]
    for groups in launches:
        flat_rows += [r for g in groups for r in g]
        flat_start += [0, len(groups[0]), len(groups[0]) + len(groups[1])]
        offs.append(len(flat_rows))
    rows_all, start_all = i32(flat_rows), i32(flat_start)
    state = hipops.DictState(K, D, DEV)
    for i in range(n_launch):
        hipops.dict_accumulate(x, rows_all[offs[i]:offs[i + 1]], start_all[3 * i:3 * i + 3], state)
    feats = torch.empty(K, D, device=DEV)
    hipops.dict_finish(state, feats=feats)
    worst = check_means(feats, x, launches, state.count.cpu())
    print('running state %d x %d: worst error %.3f of the bound' % (n_launch, max_rows, worst))
    assert state.comp.abs().max() > 0                    # the compensation term is in use


def test_one_launch_of_a_thousand_rows_runs_the_64_row_pieces():
    rs = np.random.RandomState(5)
    R, D = 1500, 16
    x = torch.from_numpy(rs.uniform(0, 1, (R, D)).astype(np.float32)).to(DEV)
    groups = [[int(r) for r in rs.randint(0, R, 1000)], [3]]
    state, feats = run(x, [groups])
    assert state.count.tolist() == [1000, 1]
    check_means(feats, x, [groups], state.count.cpu())
    assert torch.equal(feats[1], x[3])


def test_untouched_slot_is_bit_identical_and_launches_are_deterministic():
    from vln_goat_amd import hipops
    rs = np.random.RandomState(9)
    R, D, K = 300, 40, 5
    x = torch.from_numpy(rs.standard_normal((R, D)).astype(np.float32)).to(DEV)
    launches = [random_groups(rs, R, K, 90) for _ in range(6)]
    for groups in launches[3:]:
        groups[2] = []                                   # slot 2 gets nothing in the last three launches

    def sequence():
        state = hipops.DictState(K, D, DEV)
        snaps = []
        for groups in launches:
            rows, start = csr(groups)
            hipops.dict_accumulate(x, rows, start, state)
            snaps.append((state.sum.clone(), state.comp.clone(), state.count.clone()))
        return snaps
    a, b = sequence(), sequence()
    for (s0, c0, n0), (s1, c1, n1) in zip(a, b):
        assert torch.equal(s0, s1) and torch.equal(c0, c1) and torch.equal(n0, n1)
    assert a[2][0][2].any()
    for i in (3, 4, 5):                                  # compared as bits (int32 views), not as floats
        assert torch.equal(a[i][0][2].view(torch.int32), a[2][0][2].view(torch.int32))
        assert torch.equal(a[i][1][2].view(torch.int32), a[2][1][2].view(torch.int32))
        assert int(a[i][2][2]) == int(a[2][2][2])
        assert not torch.equal(a[i][0][0], a[i - 1][0][0])


# ----------------------------------------------------------------------------- finish
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_finish_writes_feats_copies_and_pz(dtype):
    from vln_goat_amd import hipops
    rs = np.random.RandomState(21)
    R, D, K, B = 120, 40, 7, 3
    x = torch.from_numpy(rs.standard_normal((R, D)).astype(np.float32)).to(DEV)
    groups = random_groups(rs, R, K, 100)
    groups[4] = []                                       # a zero-count slot
    state = hipops.DictState(K, D, DEV)
    rows, start = csr(groups)
    hipops.dict_accumulate(x, rows, start, state)
    feats = torch.full((K, D), 7.0, device=DEV)
    out = torch.full((B, K, D), 7.0, device=DEV, dtype=dtype)
    pz = torch.full((B, K, 1), 7.0, device=DEV, dtype=dtype)
    hipops.dict_finish(state, feats=feats, out=out, out_pz=pz)
    check_means(feats, x, [groups], state.count.cpu())
    assert not feats[4].any() and not out[:, 4].any() and not pz[:, 4].any()
    for b in range(B):
        assert torch.equal(out[b], feats.to(dtype)) and torch.equal(pz[b], pz[0])
    cnt = state.count.cpu().double()
    want = cnt / cnt.sum()
    if dtype == torch.float32:
        assert torch.allclose(pz[0, :, 0].cpu().double(), want, rtol=2.0 ** -23, atol=0)
    else:
        assert torch.equal(pz[0, :, 0].cpu(), want.to(torch.bfloat16))
    # each output alone, and a [B, K] pz
    f2, o2, p2 = torch.empty_like(feats), torch.empty_like(out), torch.empty(B, K, device=DEV, dtype=dtype)
    hipops.dict_finish(state, feats=f2)
    hipops.dict_finish(state, out=o2)
    hipops.dict_finish(state, out_pz=p2)
    hipops.dict_finish(state)
    assert torch.equal(f2, feats) and torch.equal(o2, out) and torch.equal(p2, pz[:, :, 0])
    with pytest.raises(ValueError):
        hipops.dict_finish(state, out=out, out_pz=p2[:2])
    with pytest.raises(ValueError):
        hipops.dict_finish(state, feats=feats[:, :8])
    with pytest.raises(ValueError):
        hipops.dict_accumulate(x[:, :24], rows, start, state)
    with pytest.raises(ValueError):
        hipops.dict_accumulate(x, rows.long(), start, state)


# ----------------------------------------------------------------------------- end to end
NAV_ARGS = dict(num_l_layers=2, num_x_layers=2, num_pano_layers=2, dropout=0.5, feat_dropout=0.4, do_back_img=False, do_back_txt=True,
                do_back_txt_type='type_2', do_front_img=False, do_front_his=False, do_front_txt=False, vocab_size=1200, mode='train')
LANDMARKS, DIRECTIONS = ['door', 'table', 'stairs', 'sofa'], ['left', 'right', 'forward']
_CACHE = {}


def nav_model_cpu(seed=11):
    from vln_goat_amd import nav_model, synth
    if seed not in _CACHE:
        model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(SimpleNamespace(**NAV_ARGS)))
        model.load_state_dict(synth.seeded_state_dict(model, seed=seed))
        _CACHE[seed] = model
    return _CACHE[seed]


def instructions(seed=3, n=9):
    """n synthetic instructions of 12-30 ids ([CLS] ... [SEP]); one token per word except a few '#' continuation pieces; every third
    word or so is a landmark or a direction (sometimes both)."""
    rs = np.random.RandomState(seed)
    data = []
    for i in range(n):
        n_tok = int(rs.randint(10, 29))
        toks = ['##x' if (j > 0 and rs.rand() < 0.15) else 'w%d' % j for j in range(n_tok)]
        n_words = sum(t[0] != '#' for t in toks)
        lm = [(w, LANDMARKS[int(rs.randint(4))]) for w in range(n_words) if rs.rand() < 0.3]
        di = [(w, DIRECTIONS[int(rs.randint(3))]) for w in range(n_words) if rs.rand() < 0.3]
        data.append({'instr_id': str(i), 'instr_encoding': [1] + [int(v) for v in rs.randint(4, 1200, n_tok)] + [2], 'tokens': toks,
                     'words': (lm, di)})
    return data


def make_plan(data, batch_size=4, kinds=('direction', 'landmark')):
    from vln_goat_amd.backdoor import InstrPickPlan
    return InstrPickPlan(data, lambda it: it['tokens'], lambda it: it['words'], batch_size=batch_size, kinds=kinds)


def host_update(model, data, batch_size, current, kinds=('direction', 'landmark')):
    """update_z_dict as the host does it: the same model calls on the same inputs, .float().cpu(), per-key Python lists, float64 means.
    current: None or {kind: (feats [K, H], pzs [K])} (device float32).  -> {kind: (keys, float64 means [K, H], mean |x| [K, H], pz dict,
    the most rows one batch gave each key)}."""
    from vln_goat_amd.backdoor import pick_positions
    lists = {k: {} for k in kinds}
    per_batch = {k: defaultdict(lambda: defaultdict(int)) for k in kinds}
    was = model.training
    model.eval()
    for i0 in range(0, len(data), batch_size):
        items = data[i0:i0 + batch_size]
        L = max(len(it['instr_encoding']) for it in items)
        ids = torch.zeros(len(items), L, dtype=torch.int64)
        mask = torch.zeros(len(items), L, dtype=torch.bool)
        for b, it in enumerate(items):
            ids[b, :len(it['instr_encoding'])] = torch.tensor(it['instr_encoding'])
            mask[b, :len(it['instr_encoding'])] = True
        inputs = defaultdict(lambda: None, {'z_txt': ids.to(DEV), 'z_txt_mask': mask.to(DEV)})
        if current is not None:
            for kind in ('direction', 'landmark'):
                f, p = current[kind]
                inputs['instr_z_%s_features' % kind] = f.unsqueeze(0).repeat(batch_size, 1, 1)[:len(items)]
                inputs['instr_z_%s_pzs' % kind] = p.view(1, -1, 1).repeat(batch_size, 1, 1)[:len(items)]
        with torch.no_grad():
            out = model('instr_zdict_update', inputs).detach().float().cpu().double().numpy()
        for b, it in enumerate(items):
            for pos, kind, key in pick_positions(it['tokens'], *it['words']):
                if kind in kinds:
                    lists[kind].setdefault(key, []).append(out[b, pos])
                    per_batch[kind][key][i0] += 1
    model.train(was)
    res = {}
    for kind in kinds:
        keys = list(lists[kind])
        total = sum(len(v) for v in lists[kind].values())
        res[kind] = (keys, np.stack([np.mean(lists[kind][k], 0) for k in keys]), np.stack([np.mean(np.abs(lists[kind][k]), 0) for k in keys]),
                     {k: len(lists[kind][k]) / total for k in keys}, [max(per_batch[kind][k].values()) for k in keys])
    return res


def assert_dictionaries(d, ret, ref, kinds=('direction', 'landmark')):
    z_dict, lm_by, di_by, lm_pz, di_pz = ret
    by, pzs = {'landmark': lm_by, 'direction': di_by}, {'landmark': lm_pz, 'direction': di_pz}
    for kind in kinds:
        keys, mean, mean_abs, pz, m = ref[kind]
        assert d.keys[kind] == keys and list(by[kind]) == keys
        assert pzs[kind] == pz                            # Python floats, count / total: equal, not close
        got = d.feats[kind].double().cpu().numpy()
        bound = (np.minimum(64, np.array(m))[:, None] + 4) * U * mean_abs
        assert (np.abs(got - mean) <= bound).all(), (kind, float((np.abs(got - mean) / bound).max()))
        assert z_dict['instr_zdict']['instr_%s_features' % kind] is d.feats[kind]
        assert torch.equal(torch.stack([by[kind][k] for k in keys]), d.feats[kind])
        want_pz = torch.tensor([pz[k] for k in keys], dtype=torch.float64)
        assert torch.allclose(d.pzs[kind].cpu().double(), want_pz, rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_update_matches_the_host_restatement_over_two_passes(dtype):
    import copy
    import vln_goat_amd
    from vln_goat_amd.backdoor import InstrDictionaries
    data = instructions()
    assert all(12 <= len(it['instr_encoding']) <= 30 for it in data)
    plan = make_plan(data)
    assert len(plan.batches) == 3 and plan.batches[-1].size == 1
    assert sorted(plan.keys['landmark']) == sorted(LANDMARKS) and sorted(plan.keys['direction']) == sorted(DIRECTIONS)
    vln_goat_amd.set_compute_dtype(dtype)
    try:
        model = copy.deepcopy(nav_model_cpu()).cuda()
        d = InstrDictionaries(DEV)
        model.train()
        ref = host_update(model, data, 4, None)
        ret = d.update(model, plan)
        assert model.training                             # the flag is put back: from train() ...
        assert_dictionaries(d, ret, ref)
        current = {k: (d.feats[k].clone(), d.pzs[k].clone()) for k in ('direction', 'landmark')}
        model.eval()
        ref2 = host_update(model, data, 4, current)
        ret2 = d.update(model, plan)                      # the second pass reads the dictionaries of the first
        assert not model.training                         # ... and from eval()
        assert_dictionaries(d, ret2, ref2)
        assert not torch.equal(d.feats['landmark'], current['landmark'][0])
        assert not np.allclose(ref2['landmark'][1], ref['landmark'][1], rtol=0, atol=1e-3)      # the dictionaries did reach the encoder
    finally:
        vln_goat_amd.set_compute_dtype(torch.float32)


def test_extras_are_rewritten_in_place_under_a_captured_graph():
    import copy
    from vln_goat_amd.backdoor import InstrDictionaries
    data = instructions()
    plan = make_plan(data)
    model = copy.deepcopy(nav_model_cpu()).cuda().eval()
    d = InstrDictionaries(DEV)
    with pytest.raises(ValueError):
        d.extras(3)                                       # nothing to hand out yet
    d.update(model, plan)
    ex, exb = d.extras(3), d.extras(2, torch.bfloat16)
    assert list(ex) == ['language'] and sorted(ex['language']) == ['instr_z_direction_features', 'instr_z_direction_pzs',
                                                                   'instr_z_landmark_features', 'instr_z_landmark_pzs']
    buf = ex['language']['instr_z_landmark_features']
    assert tuple(buf.shape) == (3, 4, 768) and tuple(ex['language']['instr_z_direction_pzs'].shape) == (3, 3, 1)
    assert torch.equal(buf, d.feats['landmark'].expand(3, 4, 768))
    ptrs = [{k: t.data_ptr() for k, t in e['language'].items()} for e in (ex, exb)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf.to(torch.bfloat16)                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # one stream, one cast: no parallel branches
        cast = buf.to(torch.bfloat16)
    graph.replay()
    assert torch.equal(cast, buf.to(torch.bfloat16))
    old = d.feats['landmark'].clone()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.05)
    d.update(model, plan)
    assert not torch.equal(d.feats['landmark'], old)
    ex2, exb2 = d.extras(3), d.extras(2, torch.bfloat16)
    assert [{k: t.data_ptr() for k, t in e['language'].items()} for e in (ex2, exb2)] == ptrs
    for kind, K in (('landmark', 4), ('direction', 3)):
        assert torch.equal(ex['language']['instr_z_%s_features' % kind], d.feats[kind].expand(3, K, 768))
        assert torch.equal(ex['language']['instr_z_%s_pzs' % kind], d.pzs[kind].view(1, K, 1).expand(3, K, 1))
        assert torch.equal(exb['language']['instr_z_%s_features' % kind], d.feats[kind].to(torch.bfloat16).expand(2, K, 768))
        assert torch.equal(exb['language']['instr_z_%s_pzs' % kind], d.pzs[kind].to(torch.bfloat16).view(1, K, 1).expand(2, K, 1))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cast, d.feats['landmark'].to(torch.bfloat16).expand(3, 4, 768))
    # another K once buffers are out: refused before anything runs, the buffers untouched
    fewer = [dict(it, words=([(w, k) for w, k in it['words'][0] if k != 'sofa'], it['words'][1])) for it in data]
    keep, keep_master = buf.clone(), d.feats['landmark'].clone()
    with pytest.raises(ValueError, match=r'3 landmark keys.*for 4'):
        d.update(model, make_plan(fewer))
    assert torch.equal(buf, keep) and torch.equal(d.feats['landmark'], keep_master)


def test_landmark_only_form_refreshes_features_and_pz(tmp_path):
    import copy
    from vln_goat_amd import features
    from vln_goat_amd.backdoor import InstrDictionaries
    data = instructions()
    plan = make_plan(data, kinds=('landmark',))
    model = copy.deepcopy(nav_model_cpu()).cuda().eval()
    d = InstrDictionaries(DEV, kinds=('landmark',))
    ref = host_update(model, data, 4, None, kinds=('landmark',))
    ret = d.update(model, plan)
    assert_dictionaries(d, ret, ref, kinds=('landmark',))
    assert ret[2] == {} and ret[4] == {} and sorted(ret[0]['instr_zdict']) == ['instr_landmark_features', 'instr_landmark_pzs']
    ex = d.extras(2)
    assert sorted(ex['language']) == ['instr_z_landmark_features', 'instr_z_landmark_pzs']
    # other picks, the same four keys: features AND pzs follow (the reference would keep the old pzs)
    other = instructions(seed=8)
    plan2 = make_plan(other, kinds=('landmark',))
    assert sorted(plan2.keys['landmark']) == sorted(LANDMARKS) and plan2.pz['landmark'] != plan.pz['landmark']
    old_pz = ex['language']['instr_z_landmark_pzs'].clone()
    ret2 = d.update(model, plan2)
    assert_dictionaries(d, ret2, host_update(model, other, 4, None, kinds=('landmark',)), kinds=('landmark',))
    assert not torch.equal(ex['language']['instr_z_landmark_pzs'], old_pz)
    assert torch.equal(ex['language']['instr_z_landmark_pzs'], d.pzs['landmark'].view(1, 4, 1).expand(2, 4, 1))
    path = str(tmp_path / 'backdoor_update_features.tsv')
    d.save_tsv(path)
    z = features.load_instr_zdict(path)
    assert torch.equal(z['instr_landmark_features'], d.feats['landmark'].cpu()) and z['instr_direction_features'].numel() == 0
    assert z['instr_landmark_pzs'].tolist() == [plan2.pz['landmark'][k] for k in d.keys['landmark']]


# ----------------------------------------------------------------------------- the image dictionary
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_image_dictionary_matches_float64_means_of_the_store(dtype, tmp_path):
    from vln_goat_amd import backdoor, features
    keys = ['scanA_vp%d' % i for i in range(7)]
    store = features.FeatureStore.synthetic(keys, D=768, seed=2, dtype=dtype).to(DEV)
    assert tuple(store.dev.shape) == (252, 768)
    rs = np.random.RandomState(6)
    labels = ['kitchen', 'hall', 'bath', 'stairs', 'porch']
    roomtypes = {k: [labels[int(v)] for v in rs.choice(5, 36, p=[0.35, 0.3, 0.2, 0.1, 0.05])] for k in reversed(keys)}
    order, counts, pz = backdoor.img_zdict_keys(roomtypes, 3)
    assert len(order) == 3
    z = backdoor.build_img_zdict(store, roomtypes, roomnum=3)
    assert z['roomtypes'] == order and z['img_pzs'].dtype == torch.float64 and z['img_pzs'].tolist() == [pz[k] for k in order]
    assert z['img_features'].is_cuda and z['img_features'].dtype == torch.float32 and tuple(z['img_features'].shape) == (3, 768)
    groups = [[store.index[k] * 36 + v for k, labs in roomtypes.items() for v, lab in enumerate(labs) if lab == name] for name in order]
    assert [len(g) for g in groups] == [counts[k] for k in order]
    check_means(z['img_features'], store.dev, [groups])
    path = str(tmp_path / 'image_z_dict_3.tsv')
    backdoor.write_img_zdict(path, z)
    back = features.load_img_zdict(path)
    assert torch.equal(back['img_features'], z['img_features'].cpu()) and torch.equal(back['img_pzs'], z['img_pzs'])
    with pytest.raises(KeyError):
        backdoor.build_img_zdict(store, {'scanB_vp0': ['hall'] * 36}, roomnum=3)
