"""The nDTW expert of RxR fine-tuning without a GPU: nav_inputs.teacher_action(expert_policy='ndtw') against the reference's own labels
(tests/golden/ndtw_expert.*, made by make_golden_ndtw_expert.py), the planner and TeacherEpisode.plan with it, the text of the label
kernel (csrc/navexpert_core.hpp) compiled as plain C++ and driven step by step beside the host planner, and the ABI of the new entry
points with the `pred` scan table."""
import json
import os

import numpy as np
import pytest
import torch

import nav_cases as N
import nav_cpu
import ndtw_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_SHAPE = -1, -2


# ---------------------------------------------------------------------------------------------------- 1. the reference's labels
def test_teacher_action_ndtw_equals_the_reference_labels():
    from vln_goat_amd import nav_inputs, rollout
    z = np.load(os.path.join(HERE, 'golden', 'ndtw_expert.npz'))
    ids = json.load(open(os.path.join(HERE, 'golden', 'ndtw_expert.json')))
    scan = rollout.ScanGraph.synthetic(**ids['scan'])
    assert scan.vpids == ids['scan_vpids'] and np.array_equal(scan.pos, z['scan_pos'])
    eps = [{'instr_id': 'ep%d' % b, 'scan': scan, 'path': ids['paths'][b], 'heading': ids['headings'][b], 'instr_encoding': ids['instr'][b]}
           for b in range(len(ids['paths']))]
    T = len(ids['steps'])
    sim, te = N.bench([scan], T, expert_policy='ndtw')
    p = rollout.EpisodePlanner(te, eps, imitation=False)
    differ = 0
    for t, st in enumerate(ids['steps']):
        part = p.build_step()
        assert p._gin['gmap_vpids'] == st['gmap_vpids'] and [tr['path'] for tr in p.traj] == st['traj']
        assert np.array_equal(p._gin['gmap_visited_masks'].numpy(), z['t%d_visited' % t]) and np.array_equal(p.ended, z['t%d_ended' % t])
        traj = [{'path': path} for path in st['traj']]
        for policy in ('ndtw', 'spl'):
            got = nav_inputs.teacher_action(p.obs, st['gmap_vpids'], z['t%d_ended' % t], z['t%d_visited' % t], False, t, -100, expert_policy=policy,
                                            traj=traj)
            assert got.dtype == np.int64 and np.array_equal(got, z['t%d_target_%s' % (t, policy)]), (t, policy, got)
        assert np.array_equal(part['s%d_target' % t].numpy(), z['t%d_target_ndtw' % t])
        real = z['t%d_target_ndtw' % t] >= 0
        differ += int((z['t%d_target_ndtw' % t][real] != z['t%d_target_spl' % t][real]).sum())
        p.advance(z['t%d_action' % t])
    assert differ >= 1


# ---------------------------------------------------------------------------------------------------- 2. planner and plan()
def test_planner_and_plan_label_with_the_chosen_expert():
    from vln_goat_amd import nav_inputs, rollout
    scans, eps = C.case_two_scans()
    T = 8
    sim, te = N.bench(scans, T, expert_policy='ndtw')
    w = N.host_walk(te, eps, N.random_policy(2, 0.05, scores=False), observe=C.observe)        # (asserts s{t}_target == teacher_action on its own state)
    parts, acts, p, stats = w.parts, w.acts, w.p, w.stats
    C.preconditions(stats)
    plan = te.plan(eps, acts)
    sim_s, te_s = N.bench(scans, T, expert_policy='spl')
    default = rollout.TeacherEpisode(sim_s, None, n_steps=T, text_len=32, pano_width=40)
    assert default.expert_policy == 'spl'
    plan_s, plan_d = te_s.plan(eps, acts), default.plan(eps, acts)
    ps = rollout.EpisodePlanner(default, eps, imitation=False)
    n = 0
    for t in range(T):
        k = 's%d_target' % t
        assert torch.equal(plan[k], parts[t][k])
        assert torch.equal(plan_s[k], plan_d[k])
        ps.build_step()
        assert np.array_equal(plan_d[k].numpy(), C.planner_labels(ps, 'spl'))
        ps.advance(acts[t])
        n += int((plan[k] != plan_d[k]).sum())
        for name in N.TABLES:                        # the expert changes the labels and nothing else
            if name != 'target':
                assert torch.equal(plan['s%d_%s' % (t, name)], plan_d['s%d_%s' % (t, name)]), (t, name)
    assert n == stats['differ'] >= 1
    assert plan['_traj'] == plan_d['_traj']
    # the teacher-forced plan (imitation labels) does not ask the expert
    assert all(torch.equal(te.plan(eps)['s%d_target' % t], default.plan(eps)['s%d_target' % t]) for t in range(T))
    with pytest.raises(ValueError, match='expert_policy'):
        rollout.TeacherEpisode(sim, None, n_steps=T, text_len=32, expert_policy='expl_sample')
    with pytest.raises(ValueError, match='expert_policy'):
        nav_inputs.teacher_action(p.obs, [[None, None]] * len(eps), np.zeros(len(eps), bool), expert_policy='dtw', traj=p.traj)
    with pytest.raises(ValueError, match='expert_policy'):
        rollout.NavRollout(None, sim, None, expert_policy='dtw')
    objects = rollout.ObjectStore.synthetic(scans[:1], D=16, max_objects=3, seed=8, dtype=torch.float32)
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    sim_o = rollout.GraphSim(rollout._RowIndex(keys), objects=objects)
    with pytest.raises(ValueError, match='shortest-path expert'):
        rollout.TeacherEpisode(sim_o, None, n_steps=T, text_len=32, expert_policy='ndtw')
    with pytest.raises(ValueError, match='shortest-path expert'):
        rollout.NavRollout(None, sim_o, None, expert_policy='ndtw')
    assert rollout.TeacherEpisode(sim_o, None, n_steps=T, text_len=32).expert_policy == 'spl'


def test_rxr_episodes_are_no_shortest_paths():
    from vln_goat_amd import rollout, synth
    scan = rollout.ScanGraph.synthetic('scanX', n=30, seed=2, degree=3)
    eps = synth.rxr_episodes(scan, np.random.RandomState(1), B=6, max_ref=10, n_way=3, starts=[0, 4, 8, 12, 16, 20])
    longer = 0
    for e, s in zip(eps, [0, 4, 8, 12, 16, 20]):
        path = e['path']
        assert path[0] == scan.vpids[s] and 1 <= len(path) <= 10 and len(set(path)) == len(path)
        assert all(scan.index[b] in scan.adj[scan.index[a]] for a, b in zip(path[:-1], path[1:]))
        longer += len(path) > len(scan.shortest_path(path[0], path[-1]))
        assert set(e) >= {'instr_id', 'scan', 'path', 'heading', 'instr_encoding'}
    assert longer >= 1


# ---------------------------------------------------------------------------------------------------- 3. the kernel's text on the CPU
@pytest.fixture(scope='module')
def cpu_kernel(tmp_path_factory):
    return nav_cpu.build(tmp_path_factory.mktemp('navexpert'))


def test_kernel_text_on_the_cpu_labels_as_the_host_planner(cpu_kernel):
    """the cases of the GPU parity test: two scans in one batch, ground-truth paths of MAX_REF, 1 and 2 viewpoints among them"""
    from vln_goat_amd.navdev import H
    h = cpu_kernel
    scans, eps = C.case_two_scans()
    T = 8
    sim, te = N.bench(scans, T, expert_policy='ndtw')
    w = N.host_walk(te, eps, N.random_policy(2, 0.05, scores=False), observe=C.observe)
    C.preconditions(w.stats)
    blocks = nav_cpu.cpu_walk(h, te, scans, eps, w, max_ref=C.MAX_REF).blocks
    assert blocks[:, H['fold']].max() > 1 and np.array_equal(blocks[:, H['ended']].astype(bool), w.p.ended)
    # without the label launch the same text gives the shortest-path labels
    sim_s, te_s = N.bench(scans, T, expert_policy='spl')
    w_s = N.host_walk(te_s, eps, lambda t, p, part: w.acts[t], observe=C.observe)
    assert all(np.array_equal(x, y) for x, y in zip(w.acts, w_s.acts))
    blocks = nav_cpu.cpu_walk(h, te_s, scans, eps, w_s).blocks
    assert not blocks[:, H['fold']].any()


# ---------------------------------------------------------------------------------------------------- 4. ABI and ScanTables
def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from vln_goat_amd import _lib
    h = _lib.lib()
    raw, p = nav_cpu.buf()

    def ndtw(scan_tab=p, step_tab=p, si=p, sd=p, log=p, ref=p, xd=p, t=1, B=2, T=3, W=40, cap=14, max_ref=12):
        return h.goat_nav_ndtw(None, scan_tab, step_tab, si, sd, log, ref, xd, t, B, T, W, cap, max_ref, -100)
    for name in ('scan_tab', 'step_tab', 'si', 'sd', 'log', 'ref', 'xd'):
        assert ndtw(**{name: None}) == E_ARG, name
    for bad in (dict(max_ref=0), dict(max_ref=65), dict(t=-1), dict(t=3), dict(B=0), dict(B=1025), dict(T=0), dict(T=65), dict(W=0), dict(W=65),
                dict(cap=0), dict(cap=255)):
        assert ndtw(**bad) == E_SHAPE, bad
    assert h.goat_nav_expert_doubles(14, 12) == (14 + 1) * (12 + 1)
    assert h.goat_nav_expert_doubles(254, 64) * 8 * 1024 < 136e6          # the ABI limits, B = 1024
    assert h.goat_nav_expert_doubles(0, 12) == 0 and h.goat_nav_expert_doubles(255, 12) == 0
    assert h.goat_nav_expert_doubles(14, 0) == 0 and h.goat_nav_expert_doubles(14, 65) == 0
    del raw


def test_scan_tables_hold_the_predecessor_matrices():
    from vln_goat_amd import navdev, navsim, rollout
    scans = [navsim.ScanGraph.synthetic('scanX', n=17, seed=2, degree=3), navsim.ScanGraph.synthetic('scanY', n=9, seed=5, degree=2)]
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    tab = rollout.ScanTables(scans, rollout._RowIndex(keys), device=None)
    assert navdev.SCAN_TABLES[:14] == ('pos', 'cand_start', 'cand_nb', 'cand_point', 'cand_ang', 'cand_len', 'feature_row', 'vp_scan', 'scan_off',
                                       'scan_n', 'dist_off', 'dist', 'vaf', 'view_ang') and navdev.SCAN_TABLES[14:] == ('pred',)
    pred_all = tab.host['pred']
    assert pred_all.dtype == np.int32 and pred_all.size == tab.host['dist'].size
    for k, sc in enumerate(scans):
        n = len(sc.vpids)
        off = int(tab.host['dist_off'][k])
        pred = pred_all[off:off + n * n].reshape(n, n)
        assert np.array_equal(pred, sc.shortest()[1])
        if n != 17:
            continue
        for a in range(n):
            for b in range(n):
                chain = [b]
                while chain[-1] != a:
                    chain.append(int(pred[a, chain[-1]]))
                    assert len(chain) <= n
                assert [sc.vpids[i] for i in reversed(chain)] == sc.shortest_path(sc.vpids[a], sc.vpids[b])


def test_device_navigator_checks_the_expert_before_it_touches_the_device():
    from vln_goat_amd import rollout
    te = type('TE', (), {'objects': None, 'expert_policy': 'dtw'})()
    with pytest.raises(ValueError, match='expert_policy'):
        rollout.DeviceNavigator(te, None, None, 'sample')
    te = type('TE', (), {'objects': None, 'expert_policy': 'ndtw'})()
    for bad in (0, 65):
        with pytest.raises(ValueError, match='max_ref'):
            rollout.DeviceNavigator(te, None, None, 'sample', max_ref=bad)
