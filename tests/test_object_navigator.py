"""The device navigator of REVERIE / SOON walks without a GPU: navdev.ObjectTables against ObjectStore.attributes, the text of the
kernels (csrc/navstate_core.hpp with Args::O > 0) compiled as plain C++ and driven step by step beside EpisodePlanner with objects in
forced and argmax mode, the argument checks of the goat_nav_obj_* entry points, and the host helper that stages the goals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import object_nav_cases as C

E_ARG, E_SHAPE = -1, -2
GUARD = 64          # elements in front of and behind every buffer the kernel text writes; nothing may touch them


# ---------------------------------------------------------------------------------------------------- 1. ObjectTables
def test_object_tables_pack_what_attributes_returns():
    from vln_goat_amd import navdev, navsim, rollout
    scans, objects = C.scans_and_objects()
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    tables = rollout.ScanTables(scans, rollout._RowIndex(keys), device=None)
    ot = rollout.ObjectTables(objects, tables, device=None)
    om = navdev.ObjectTables(objects.meta(), tables, device=None)
    assert navdev.OBJECT_TABLES == ('obj_start', 'obj_row', 'obj_dir', 'obj_box', 'obj_name')
    assert ot.tab is None and set(ot.host) == set(navdev.OBJECT_TABLES)
    for name in navdev.OBJECT_TABLES:
        assert ot.host[name].dtype == om.host[name].dtype and np.array_equal(ot.host[name], om.host[name]), name
    assert ot.ids == om.ids
    h = ot.host
    assert h['obj_start'].dtype == np.int32 and h['obj_row'].dtype == np.int32 and h['obj_dir'].dtype == np.float64
    assert h['obj_box'].dtype == np.float32 and h['obj_name'].dtype == np.int64
    seen = 0
    for sc in scans:
        for vp in sc.vpids:
            v = tables.vp(sc.name, vp)
            lo, hi = int(h['obj_start'][v]), int(h['obj_start'][v + 1])
            for bh, be in ((0.0, 0.0), (2.6179938779914944, -0.5235987755982988)):
                rows, ang, box, ids, names = objects.attributes(sc.name, vp, bh, be, 4)
                assert hi - lo == len(rows) and list(ids) == ot.ids[v]
                assert np.array_equal(rows, h['obj_row'][v] + np.arange(hi - lo))
                assert np.array_equal(box, h['obj_box'][lo:hi]) and np.array_equal(np.asarray(names, np.int64), h['obj_name'][lo:hi])
                mine = np.zeros((hi - lo, 4), np.float32)
                for j in range(hi - lo):
                    mine[j] = navsim.angle_feature(h['obj_dir'][lo + j, 0] - bh, h['obj_dir'][lo + j, 1] - be, 4)
                assert np.array_equal(mine, ang)
            seen += hi - lo
    assert seen == h['obj_dir'].shape[0] == h['obj_box'].shape[0] == h['obj_name'].shape[0] > 0
    assert (np.diff(h['obj_start']) == 0).any() and (np.diff(h['obj_start']) == 5).any()


# ---------------------------------------------------------------------------------------------------- 2. the kernel's text on the CPU
WRAPPER = r'''
#include <vector>
#include "navstate_core.hpp"
using namespace navstate;
struct NoSync { void operator()() const {} };
extern "C" {
int cpu_state_ints(int T, int W, int O, int cap) { return Layout(cap, T, W, O).ints; }
int cpu_log_ints(int T, int cap) { return Layout(cap, T, 1).log_ints; }
int cpu_small_ints(int T, int W, int O, int cap) { return Layout(cap, T, W, O).small + HDR; }
void cpu_reset(const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B, int T, int W, int O, int cap) {
  Args a = {};
  a.scan_tab = scan_tab; a.si = si; a.sd = sd; a.log = log; a.B = B; a.T = T; a.W = W; a.cap = cap; a.O = O;
  for (int b = 0; b < B; ++b) reset_episode(a, ep, b, 0, 1, NoSync());
}
void cpu_step(const int64_t* scan_tab, const int64_t* obj_tab, const int64_t* step_tab, const int64_t* ostep_tab, int32_t* si, double* sd,
              int32_t* log, int32_t* ws, const void* act, const int32_t* goal, int mode, int t, int B, int T, int Gp, int G, int W, int O,
              int max_end, int A, int cap, int64_t ignoreid) {
  Args a = {scan_tab, step_tab, si, sd, log, ws, act, nullptr, mode, t, B, T, Gp, G, W, A, cap, ignoreid, obj_tab, ostep_tab, goal, O, max_end};
  std::vector<int32_t> staged(Layout(cap, T, W, O).small + HDR);        // odd episodes: with the staged copy a kernel keeps in LDS
  for (int b = 0; b < B; ++b) step_episode(a, b, 0, 1, NoSync(), b % 2 ? staged.data() : nullptr);
  if (t >= T) return;
  int32_t part[1];
  nav_tail(a, part, 0, 1, NoSync());
}
}
'''


@pytest.fixture(scope='module')
def cpu_kernel(tmp_path_factory):
    from vln_goat_amd import _lib
    d = tmp_path_factory.mktemp('navobj')
    src, so = str(d / 'wrapper.cpp'), str(d / 'libnavobj_cpu.so')
    open(src, 'w').write(WRAPPER)
    cmd = [os.environ.get('CXX', 'c++'), '-O1', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-I', _lib.CSRC, src, '-o', so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    h = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    h.cpu_reset.argtypes, h.cpu_reset.restype = [vp] * 5 + [i32] * 5, None
    h.cpu_step.argtypes, h.cpu_step.restype = [vp] * 10 + [i32] * 11 + [ctypes.c_int64], None
    return h


def _addr(a):
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data


class _Guarded:
    """an array between two guard bands of a value the kernel text never writes there"""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.all = np.full(n + 2 * GUARD, fill, dtype)
        self.a = self.all[GUARD:GUARD + n].reshape(shape)
        self.fill = fill

    def intact(self):
        f = np.asarray(self.fill, self.all.dtype)
        return bool((self.all[:GUARD] == f).all() and (self.all[GUARD + self.a.size:] == f).all())


def _cpu_device_walk(h, te, scans, objects, eps, mode, acts, scores, bests, parts, max_end=4):
    """reset / step / tail of the kernels' text on one thread over host memory in `mode`; every step's tables against the host
    planner's -> (the read-back blocks, the actions and alive flags of the log)"""
    from vln_goat_amd import navdev, rollout
    B, T, W, O = len(eps), te.T, te.W, te.O
    tables = rollout.ScanTables(scans, te.sim.features, device=None)
    ot = rollout.ObjectTables(objects, tables, device=None)
    scan_tab = np.array([_addr(tables.host[name]) for name in navdev.SCAN_TABLES], np.int64)
    obj_tab = np.array([_addr(ot.host[name]) for name in navdev.OBJECT_TABLES], np.int64)
    gw = [int(te.gw(t)) for t in range(T)]
    cap = max(gw) - 2
    ints = h.cpu_state_ints(T, W, O, cap)
    assert ints == h.cpu_state_ints(T, W, 0, cap) + cap and h.cpu_small_ints(T, W, O, cap) == h.cpu_small_ints(T, W, 0, cap) + cap
    si = _Guarded((B * ints,), np.int32, 0x55555555)
    sd = _Guarded((B * (cap * cap + cap),), np.float64, 7.25)
    log_ints = h.cpu_log_ints(T, cap)
    log = _Guarded((2 * T * B + B * log_ints,), np.int32, 0x55555555)
    ws = _Guarded((2 * (B + 1) + T * (B * (W + O) + B) + B + 1 + B + 1,), np.int32, 0x55555555)
    goal = _Guarded((B, max_end, 2), np.int32, 0x55555555)
    goal.a[:] = navdev.object_goals(eps, ot, max_end, te.sim.obj_fallback)
    ep = np.zeros((B, 4), np.int32)
    for i, e in enumerate(eps):
        name = e['scan'].name
        ep[i] = (tables.ids[name], tables.vp(name, e['path'][0]), rollout.GraphSim._snap(e['heading'], 0.0), tables.vp(name, e['path'][-1]))
    forced = np.zeros((T, B), np.int32)
    forced[:len(acts)] = np.asarray(acts)
    back = np.zeros((3, B), np.float32)
    h.cpu_reset(_addr(scan_tab), _addr(si.a), _addr(sd.a), _addr(log.a), _addr(ep), B, T, W, O, cap)
    names = C.TABLES + C.OBJECT_TABLES
    for t in range(T + 1):
        if t < T:
            step = {}
            for name in names:
                w = parts[t]['s%d_%s' % (t, name)].numpy()
                step[name] = _Guarded(w.shape, w.dtype, 85)
                step[name].a[...] = 77
            step_tab = np.array([_addr(step[name].a) for name in C.TABLES], np.int64)
            ostep_tab = np.array([_addr(step[name].a) for name in C.OBJECT_TABLES], np.int64)
        if t > 0 and mode == 'argmax':
            back[:] = np.stack([acts[t - 1].astype(np.float32), scores[t - 1], bests[t - 1]])
        act = forced if mode == 'forced' else back
        h.cpu_step(_addr(scan_tab), _addr(obj_tab), _addr(step_tab) if t < T else None, _addr(ostep_tab) if t < T else None, _addr(si.a),
                   _addr(sd.a), _addr(log.a), _addr(ws.a), _addr(act), _addr(goal.a), navdev.MODES[mode], t, B, T,
                   gw[t - 1] if t > 0 else 0, gw[t] if t < T else 0, W, O, max_end, C.A, cap, -100)
        if t < T:
            C.compare(t, {'s%d_%s' % (t, name): torch.from_numpy(step[name].a) for name in names}, parts[t])
            assert all(step[name].intact() for name in names), [name for name in names if not step[name].intact()]
    assert si.intact() and sd.intact() and log.intact() and ws.intact() and goal.intact()
    blocks = log.a[2 * T * B:].reshape(B, log_ints)
    assert not blocks[:, 5].any(), blocks[:, 5:7]
    return blocks, log.a[:T * B].reshape(T, B), ot


@pytest.fixture(scope='module')
def case():
    scans, objects = C.scans_and_objects()
    eps = C.episodes(scans, objects)
    sim, te = C.bench(scans, objects)
    return scans, objects, eps, te


def test_kernel_text_on_the_cpu_builds_the_object_tables_of_a_forced_walk(cpu_kernel, case):
    scans, objects, eps, te = case
    parts, acts, scores, bests, ended, p, stats = C.host_walk(te, eps, C.policy(2))
    C.preconditions(stats, ended)
    blocks, log_acts, _ = _cpu_device_walk(cpu_kernel, te, scans, objects, eps, 'forced', acts, scores, bests, parts)
    assert np.array_equal(blocks[:, 2].astype(bool), p.ended) and int(blocks[:, 11].sum()) == p.n_traj
    assert np.array_equal(log_acts, np.asarray(acts))
    assert not blocks[:, 22:24].any()           # no object record outside argmax mode


def test_kernel_text_on_the_cpu_records_the_best_objects_of_an_argmax_walk(cpu_kernel, case):
    scans, objects, eps, te = case
    parts, acts, scores, bests, ended, p, stats = C.host_walk(te, eps, C.policy(2, tie=(1, (0, 1), 0.5)), feedback='argmax')
    C.preconditions(stats, ended)
    want = [tr['pred_objid'] for tr in p.traj]
    assert any(x is None for x in want) and any(x is not None for x in want), want
    blocks, _, ot = _cpu_device_walk(cpu_kernel, te, scans, objects, eps, 'argmax', acts, scores, bests, parts)
    assert np.array_equal(blocks[:, 2].astype(bool), p.ended)
    got = [ot.ids[int(v) - 1][int(j)] if (v > 0 and j >= 0) else None for v, j in blocks[:, 22:24]]
    assert got == want


# ---------------------------------------------------------------------------------------------------- 3. ABI
def _buf():
    raw = (ctypes.c_char * 4096)()
    return raw, ctypes.addressof(raw) & ~63


def test_object_entry_points_reject_bad_arguments_before_any_launch():
    from vln_goat_amd import _lib
    h = _lib.lib()
    raw, p = _buf()

    def step(scan_tab=p, obj_tab=p, step_tab=p, ostep_tab=p, si=p, sd=p, log=p, ws=p, act=p, u=p, goal=p, mode=0, t=1, B=2, T=3, Gp=16, G=16,
             W=40, O=5, max_end=4, A=4, cap=14):
        return h.goat_nav_obj_step(None, scan_tab, obj_tab, step_tab, ostep_tab, si, sd, log, ws, act, u, goal, mode, t, B, T, Gp, G, W, O,
                                   max_end, A, cap, -100)

    def reset(scan_tab=p, si=p, sd=p, log=p, ep=p, B=2, T=3, W=40, O=5, cap=14):
        return h.goat_nav_obj_reset(None, scan_tab, si, sd, log, ep, B, T, W, O, cap)
    for name in ('scan_tab', 'obj_tab', 'step_tab', 'ostep_tab', 'si', 'sd', 'log', 'ws', 'act', 'u', 'goal'):
        assert step(**{name: None}) == E_ARG, name
    assert step(mode=3) == E_ARG
    for bad in (dict(O=0), dict(O=65), dict(max_end=0), dict(max_end=65), dict(t=-1), dict(t=4), dict(B=0), dict(B=1025), dict(T=0), dict(T=65),
                dict(W=0), dict(W=65), dict(cap=0), dict(cap=255), dict(G=1), dict(G=17), dict(G=257), dict(Gp=1), dict(Gp=257), dict(A=3),
                dict(A=68)):
        assert step(**bad) == E_SHAPE, bad
    for name in ('scan_tab', 'si', 'sd', 'log', 'ep'):
        assert reset(**{name: None}) == E_ARG, name
    for bad in (dict(O=0), dict(O=65), dict(B=0), dict(B=1025), dict(T=0), dict(T=65), dict(W=0), dict(W=65), dict(cap=0), dict(cap=255)):
        assert reset(**bad) == E_SHAPE, bad
    ints = h.goat_nav_obj_state_ints(6, 40, 5, 14)
    assert ints == h.goat_nav_state_ints(6, 40, 14) + 14
    for bad in ((6, 40, 0, 14), (6, 40, 65, 14), (0, 40, 5, 14), (65, 40, 5, 14), (6, 0, 5, 14), (6, 65, 5, 14), (6, 40, 5, 0), (6, 40, 5, 255)):
        assert h.goat_nav_obj_state_ints(*bad) == 0, bad
    assert h.goat_nav_obj_state_ints(64, 64, 64, 254) > 0
    del raw


# ---------------------------------------------------------------------------------------------------- 4. the goals
def test_object_goals_follow_the_first_match_rule():
    from vln_goat_amd import navdev, rollout
    scans, objects = C.scans_and_objects()
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    tables = rollout.ScanTables(scans, rollout._RowIndex(keys), device=None)
    ot = rollout.ObjectTables(objects, tables, device=None)
    sc = scans[0]
    full = [vp for vp in sc.vpids if len(ot.ids[tables.vp(sc.name, vp)]) >= 2]
    empty = [vp for vp in sc.vpids if not ot.ids[tables.vp(sc.name, vp)]]
    assert full and empty
    v = tables.vp(sc.name, full[0])
    ot.ids[v] = [str(ot.ids[v][1])] + list(ot.ids[v][1:])          # the second id twice, once as a string: the first match wins
    target = ot.ids[v][1]
    base = {'scan': sc, 'path': [full[0]], 'heading': 0.0, 'instr_encoding': [1], 'instr_id': 'g'}
    eps = [dict(base, obj_id=target, end_vps=[empty[0], full[0], full[0]]), dict(base, obj_id=C.ABSENT, end_vps=[full[0]]),
           dict(base, obj_id=None, end_vps=[full[0], empty[0]]), dict(base, obj_id=target)]
    g = navdev.object_goals(eps, ot, 3)
    assert g.dtype == np.int32 and g.shape == (4, 3, 2)
    assert g[0].tolist() == [[tables.vp(sc.name, empty[0]), -1], [v, 0], [v, 0]]
    assert g[1].tolist() == [[v, -1], [-1, -1], [-1, -1]]
    assert g[2].tolist() == [[v, -1], [tables.vp(sc.name, empty[0]), -1], [-1, -1]]
    assert g[3].tolist() == [[-1, -1]] * 3
    with pytest.raises(ValueError, match='max_end'):
        navdev.object_goals(eps, ot, 2)
    with pytest.raises(ValueError, match='obj_id'):
        navdev.object_goals(eps, ot, 3, obj_fallback=True)
    assert navdev.object_goals([eps[0], eps[1]], ot, 3, obj_fallback=True).shape == (2, 3, 2)


# ---------------------------------------------------------------------------------------------------- 5. the constructor
def test_device_navigator_asks_for_the_object_tables():
    from vln_goat_amd import rollout
    scans, objects = C.scans_and_objects()
    sim, te = C.bench(scans, objects)
    with pytest.raises(NotImplementedError, match='ObjectTables'):
        rollout.DeviceNavigator(te, None, None, 'sample')
    with pytest.raises(NotImplementedError, match='ObjectTables'):
        rollout.DeviceNavigator(te, None, None, 'sample', objects=None, max_end=8)
