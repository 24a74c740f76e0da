"""The device navigator of REVERIE / SOON walks without a GPU: navdev.ObjectTables against ObjectStore.attributes, the text of the
kernels (csrc/navstate_core.hpp with Args::O > 0) compiled as plain C++ and driven step by step beside EpisodePlanner with objects in
forced and argmax mode, the argument checks of the goat_nav_obj_* entry points, and the host helper that stages the goals."""
import numpy as np
import pytest

import nav_cases as N
import nav_cpu
import object_nav_cases as C
from vln_goat_amd.navdev import H

E_ARG, E_SHAPE = -1, -2


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
@pytest.fixture(scope='module')
def cpu_kernel(tmp_path_factory):
    return nav_cpu.build(tmp_path_factory.mktemp('navobj'))


@pytest.fixture(scope='module')
def case():
    scans, objects = C.scans_and_objects()
    eps = C.episodes(scans, objects)
    sim, te = C.bench(scans, objects)
    return scans, objects, eps, te


def test_kernel_text_on_the_cpu_builds_the_object_tables_of_a_forced_walk(cpu_kernel, case):
    scans, objects, eps, te = case
    w = N.host_walk(te, eps, C.policy(2), observe=C.observe)
    C.preconditions(w.stats, w.ended)
    got = nav_cpu.cpu_walk(cpu_kernel, te, scans, eps, w, 'forced', objects=objects)
    assert np.array_equal(got.blocks[:, H['ended']].astype(bool), w.p.ended) and int(got.blocks[:, H['live']].sum()) == w.p.n_traj
    assert np.array_equal(got.acts, np.asarray(w.acts))
    assert not got.blocks[:, H['pred_vp']:H['pred_obj'] + 1].any()           # no object record outside argmax mode


def test_kernel_text_on_the_cpu_records_the_best_objects_of_an_argmax_walk(cpu_kernel, case):
    scans, objects, eps, te = case
    w = N.host_walk(te, eps, C.policy(2, tie=(1, (0, 1), 0.5)), 'argmax', C.observe)
    C.preconditions(w.stats, w.ended)
    want = [tr['pred_objid'] for tr in w.p.traj]
    assert any(x is None for x in want) and any(x is not None for x in want), want
    got = nav_cpu.cpu_walk(cpu_kernel, te, scans, eps, w, 'argmax', objects=objects)
    assert np.array_equal(got.blocks[:, H['ended']].astype(bool), w.p.ended)
    assert [got.ot.ids[int(v) - 1][int(j)] if (v > 0 and j >= 0) else None for v, j in got.blocks[:, H['pred_vp']:H['pred_obj'] + 1]] == want


# ---------------------------------------------------------------------------------------------------- 3. ABI
def test_object_entry_points_reject_bad_arguments_before_any_launch():
    from vln_goat_amd import _lib
    h = _lib.lib()
    raw, p = nav_cpu.buf()

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
