"""The nDTW expert of RxR fine-tuning without a GPU: nav_inputs.teacher_action(expert_policy='ndtw') against the reference's own labels
(tests/golden/ndtw_expert.*, made by make_golden_ndtw_expert.py), the planner and TeacherEpisode.plan with it, the text of the label
kernel (csrc/navexpert_core.hpp) compiled as plain C++ and driven step by step beside the host planner, and the ABI of the new entry
points with the `pred` scan table."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

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
    sim, te = C.bench([scan], T)
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
    sim, te = C.bench(scans, T)
    parts, acts, p, stats = C.host_walk(te, eps, C.random_policy(2, 0.05))        # (asserts s{t}_target == teacher_action on its own state)
    C.preconditions(stats)
    plan = te.plan(eps, acts)
    sim_s, te_s = C.bench(scans, T, expert_policy='spl')
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
        for name in C.TABLES:                        # the expert changes the labels and nothing else
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
WRAPPER = r'''
#include "navexpert_core.hpp"
using namespace navstate;
struct NoSync { void operator()() const {} };
extern "C" {
int cpu_state_ints(int T, int W, int cap) { return Layout(cap, T, W).ints; }
int cpu_log_ints(int T, int cap) { return Layout(cap, T, 1).log_ints; }
int cpu_expert_doubles(int cap, int max_ref) { return expert_doubles(cap, max_ref); }
void cpu_reset(const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B, int T, int W, int cap) {
  Args a = {};
  a.scan_tab = scan_tab; a.si = si; a.sd = sd; a.log = log; a.B = B; a.T = T; a.W = W; a.cap = cap;
  for (int b = 0; b < B; ++b) reset_episode(a, ep, b, 0, 1, NoSync());
}
void cpu_step(const int64_t* scan_tab, const int64_t* step_tab, int32_t* si, double* sd, int32_t* log, int32_t* ws, const int32_t* act,
              int t, int B, int T, int Gp, int G, int W, int A, int cap, int64_t ignoreid, const int32_t* ref, double* xd, int max_ref) {
  Args a = {scan_tab, step_tab, si, sd, log, ws, act, nullptr, MODE_FORCED, t, B, T, Gp, G, W, A, cap, ignoreid};
  for (int b = 0; b < B; ++b) step_episode(a, b, 0, 1, NoSync());
  if (t >= T) return;
  int32_t part[1];
  nav_tail(a, part, 0, 1, NoSync());
  const Expert x = {ref, xd, max_ref};
  double row_s[65];          // odd episodes: with the staged copies a kernel keeps in LDS
  int32_t ref_s[65];
  if (ref)
    for (int b = 0; b < B; ++b) ndtw_label(a, x, b, 0, 1, NoSync(), b % 2 ? row_s : nullptr, b % 2 ? ref_s : nullptr);
}
}
'''


@pytest.fixture(scope='module')
def cpu_kernel(tmp_path_factory):
    from vln_goat_amd import _lib
    d = tmp_path_factory.mktemp('navexpert')
    src, so = str(d / 'wrapper.cpp'), str(d / 'libnavexpert_cpu.so')
    open(src, 'w').write(WRAPPER)
    cmd = [os.environ.get('CXX', 'c++'), '-O1', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-I', _lib.CSRC, src, '-o', so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    h = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    h.cpu_reset.argtypes, h.cpu_reset.restype = [vp] * 5 + [i32] * 4, None
    h.cpu_step.argtypes, h.cpu_step.restype = [vp] * 7 + [i32] * 8 + [ctypes.c_int64, vp, vp, i32], None
    return h


def _addr(a):
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data


def _cpu_device_walk(h, te, scans, eps, acts, parts, max_ref, expert=True):
    """reset / step / tail / label of the kernels' text on one thread over host memory, every step's tables against the host planner's"""
    from vln_goat_amd import navdev, rollout
    B, T, W = len(eps), te.T, te.W
    tables = rollout.ScanTables(scans, te.sim.features, device=None)
    scan_tab = np.array([_addr(tables.host[name]) for name in navdev.SCAN_TABLES], np.int64)
    gw = [int(te.gw(t)) for t in range(T)]
    cap = max(gw) - 2
    si = np.zeros(B * h.cpu_state_ints(T, W, cap), np.int32)
    sd = np.zeros(B * (cap * cap + cap), np.float64)
    log_ints = h.cpu_log_ints(T, cap)
    log = np.zeros(2 * T * B + B * log_ints, np.int32)
    ws = np.zeros(2 * (B + 1) + T * (B * W + B) + B + 1, np.int32)
    GUARD = 64                  # words in front of and behind the expert's rows that nothing may write
    xd_all = np.full(B * h.cpu_expert_doubles(cap, max_ref) + 2 * GUARD, np.nan)
    xd = xd_all[GUARD:-GUARD]
    ref = np.zeros((B, max_ref + 1), np.int32)
    ep = np.zeros((B, 4), np.int32)
    for i, e in enumerate(eps):
        name = e['scan'].name
        ep[i] = (tables.ids[name], tables.vp(name, e['path'][0]), rollout.GraphSim._snap(e['heading'], 0.0), tables.vp(name, e['path'][-1]))
        ref[i, 0] = len(e['path'])
        ref[i, 1:1 + len(e['path'])] = [tables.vp(name, vp) for vp in e['path']]
    forced = np.zeros((T, B), np.int32)
    forced[:len(acts)] = np.asarray(acts)
    h.cpu_reset(_addr(scan_tab), _addr(si), _addr(sd), _addr(log), _addr(ep), B, T, W, cap)
    for t in range(T + 1):
        if t < T:
            step = {name: np.full_like(parts[t]['s%d_%s' % (t, name)].numpy(), 85) for name in C.TABLES}
            step_tab = np.array([_addr(step[name]) for name in C.TABLES], np.int64)
        h.cpu_step(_addr(scan_tab), _addr(step_tab) if t < T else None, _addr(si), _addr(sd), _addr(log), _addr(ws), _addr(forced), t, B, T,
                   gw[t - 1] if t > 0 else 0, gw[t] if t < T else 0, W, C.A, cap, -100, _addr(ref) if expert else None, _addr(xd),
                   max_ref)
        if t < T:
            C.compare(t, {'s%d_%s' % (t, name): torch.from_numpy(v) for name, v in step.items()}, parts[t])
    assert np.isnan(xd_all[:GUARD]).all() and np.isnan(xd_all[-GUARD:]).all()
    blocks = log[2 * T * B:].reshape(B, log_ints)
    assert not blocks[:, 5].any(), blocks[:, 5:7]
    return blocks


def test_kernel_text_on_the_cpu_labels_as_the_host_planner(cpu_kernel):
    """the cases of the GPU parity test: two scans in one batch, ground-truth paths of MAX_REF, 1 and 2 viewpoints among them"""
    h = cpu_kernel
    scans, eps = C.case_two_scans()
    T = 8
    sim, te = C.bench(scans, T)
    parts, acts, p, stats = C.host_walk(te, eps, C.random_policy(2, 0.05))
    C.preconditions(stats)
    blocks = _cpu_device_walk(h, te, scans, eps, acts, parts, C.MAX_REF)
    assert blocks[:, 21].max() > 1 and np.array_equal(blocks[:, 2].astype(bool), p.ended)
    # without the label launch the same text gives the shortest-path labels
    sim_s, te_s = C.bench(scans, T, expert_policy='spl')
    parts_s, acts_s, _, _ = C.host_walk(te_s, eps, lambda t, p, part: acts[t])
    assert all(np.array_equal(x, y) for x, y in zip(acts, acts_s))
    blocks = _cpu_device_walk(h, te_s, scans, eps, acts, parts_s, C.MAX_REF, expert=False)
    assert not blocks[:, 21].any()


# ---------------------------------------------------------------------------------------------------- 4. ABI and ScanTables
def _buf():
    raw = (ctypes.c_char * 4096)()
    return raw, ctypes.addressof(raw) & ~63


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from vln_goat_amd import _lib
    h = _lib.lib()
    raw, p = _buf()

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
