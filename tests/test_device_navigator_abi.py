"""The device navigator without a GPU: goat_nav_reset / goat_nav_step reject null pointers and impossible sizes before any launch,
navdev.ScanTables packs a scan exactly as the host navigator reads it (candidate order, pointId, angles, shortest distances, and the edge
lengths GraphMap.update_graph would compute, bit for bit), navdev names the header words and lays out the workspace as the kernels do,
and the kernels' text compiled as plain C++ (nav_cpu.py) samples its actions as SampledEpisode.sample does."""
import numpy as np
import pytest

import nav_cases as N
import nav_cpu

E_ARG, E_SHAPE = -1, -2


def test_entry_points_reject_bad_arguments_before_any_launch():
    from vln_goat_amd import _lib
    h = _lib.lib()
    raw, p = nav_cpu.buf()
    B, T, W, cap = 2, 3, 40, 14
    ok_reset = dict(scan_tab=p, si=p, sd=p, log=p, ep=p)
    for name in ok_reset:
        a = dict(ok_reset, **{name: None})
        assert h.goat_nav_reset(None, a['scan_tab'], a['si'], a['sd'], a['log'], a['ep'], B, T, W, cap) == E_ARG, name
    for bad in (dict(B=0), dict(B=1025), dict(T=0), dict(T=65), dict(W=0), dict(W=65), dict(cap=0), dict(cap=255)):
        s = {**dict(B=B, T=T, W=W, cap=cap), **bad}
        assert h.goat_nav_reset(None, p, p, p, p, p, s['B'], s['T'], s['W'], s['cap']) == E_SHAPE, bad

    def step(scan_tab=p, step_tab=p, si=p, sd=p, log=p, ws=p, act=p, u=p, mode=0, t=1, B=B, T=T, Gp=16, G=16, W=W, A=4, cap=cap):
        return h.goat_nav_step(None, scan_tab, step_tab, si, sd, log, ws, act, u, mode, t, B, T, Gp, G, W, A, cap, -100)
    for name in ('scan_tab', 'step_tab', 'si', 'sd', 'log', 'ws', 'act', 'u'):
        assert step(**{name: None}) == E_ARG, name
    assert step(mode=3) == E_ARG and step(mode=-1) == E_ARG
    for bad in (dict(B=0), dict(B=1025), dict(T=0), dict(T=65), dict(G=0), dict(G=257), dict(G=17), dict(Gp=0), dict(Gp=257), dict(W=0),
                dict(W=65), dict(cap=0), dict(cap=255), dict(t=-1), dict(t=4), dict(A=0), dict(A=6)):
        assert step(**bad) == E_SHAPE, bad
    assert h.goat_nav_state_ints(T, W, cap) > cap * cap and h.goat_nav_log_ints(T, cap) >= 32 + T + 2 + (T + 1) * cap
    assert h.goat_nav_state_ints(0, W, cap) == 0 and h.goat_nav_state_ints(T, W, 255) == 0 and h.goat_nav_log_ints(65, cap) == 0
    del raw


def test_scan_tables_pack_what_the_host_navigator_reads():
    from vln_goat_amd import navsim, rollout
    scans = [navsim.ScanGraph.synthetic('scanX', n=17, seed=2, degree=3), navsim.ScanGraph.synthetic('scanY', n=9, seed=5, degree=2)]
    keys = ['%s_%s' % (sc.name, vp) for sc in reversed(scans) for vp in sc.vpids]         # (feature rows in another order than the tables)
    rows = rollout._RowIndex(keys)
    tab = rollout.ScanTables(scans, rows, device=None)
    h = tab.host
    assert tab.dev is None and h['pos'].dtype == np.float64 and h['cand_len'].dtype == np.float64 and h['dist'].dtype == np.float64
    assert h['scan_off'].tolist() == [0, 17] and h['scan_n'].tolist() == [17, 9] and h['dist_off'].tolist() == [0, 17 * 17]
    assert np.array_equal(h['vaf'], navsim.view_angle_feature_table(4)) and h['vaf'].dtype == np.float32
    assert h['view_ang'].tolist() == [list(navsim.view_angles(v)) for v in range(36)]
    n_cand = 0
    for k, sc in enumerate(scans):
        off = int(h['scan_off'][k])
        dist = h['dist'][int(h['dist_off'][k]):int(h['dist_off'][k]) + len(sc.vpids) ** 2].reshape(len(sc.vpids), -1)
        assert np.array_equal(dist, sc.shortest()[0])
        sim = navsim.GraphSim(rows)
        for i, vp in enumerate(sc.vpids):
            v = off + i
            assert tab.vp(sc.name, vp) == v and tab.names[v] == vp
            assert h['pos'][v].tolist() == list(sc.pos[i]) and h['feature_row'][v] == rows.row(sc.name, vp) and h['vp_scan'][v] == k
            c0, c1 = int(h['cand_start'][v]), int(h['cand_start'][v + 1])
            cands = sc.candidates(vp)
            assert c1 - c0 == len(cands)
            # the edge lengths the map would hold after update_graph on this viewpoint's observation
            ob = sim.reset([{'instr_id': 'x', 'scan': sc, 'path': [vp], 'heading': 0.0, 'instr_encoding': [0, 2]}])[0]
            g = navsim.GraphMap(vp)
            g.update_graph(ob)
            for j, c in enumerate(cands):
                assert tab.names[h['cand_nb'][c0 + j]] == c['viewpointId'] and h['cand_point'][c0 + j] == c['pointId']
                assert h['cand_ang'][c0 + j, 0] == c['normalized_heading'] and h['cand_ang'][c0 + j, 1] == c['normalized_elevation']
                want = g.graph.D[g.graph.ids[vp], g.graph.ids[c['viewpointId']]]
                assert h['cand_len'][c0 + j] == want, (vp, j, h['cand_len'][c0 + j], want)
            n_cand += len(cands)
    assert n_cand == len(h['cand_nb']) > 0


def test_device_navigator_keeps_object_walks_on_the_host():
    from vln_goat_amd import rollout
    te = type('TE', (), {'objects': object()})()
    with pytest.raises(NotImplementedError):
        rollout.DeviceNavigator(te, None, None, 'sample')


# ---------------------------------------------------------------------------------------------------- the kernels' text on the CPU
@pytest.fixture(scope='module')
def cpu_kernel(tmp_path_factory):
    return nav_cpu.build(tmp_path_factory.mktemp('navstate'))


def test_navdev_names_the_header_words_and_lays_out_the_workspace_as_the_kernels_do(cpu_kernel):
    from vln_goat_amd import navdev
    h = cpu_kernel
    assert navdev.HDR == h.cpu_header_ints() >= len(navdev.HEADER) == len(set(navdev.HEADER))
    for i, name in enumerate(navdev.HEADER):
        assert h.cpu_header_word(name.upper().encode()) == i == navdev.H[name], name
    assert h.cpu_header_word(b'NO_SUCH_WORD') == -1
    for B, T, W, O in ((1, 1, 1, 0), (5, 8, 40, 0), (6, 6, 40, 5), (12, 15, 40, 1), (1024, 64, 64, 0), (1024, 64, 64, 64)):
        assert navdev.workspace(B, T, W, O) == (h.cpu_ws_ints(B, T, W, O), h.cpu_ws_live_at(B, T, W, O)), (B, T, W, O)


SAMPLE_SEED = 0          # chosen on the host planner alone: a multi-hop move, and an episode still walking at T - 1


def test_kernel_text_on_the_cpu_samples_as_the_host_planner_does(cpu_kernel):
    """An R2R walk in 'sample' mode, B = 5, T = 8, over the two scans of ndtw_cases.case_two_scans: per step a seeded random float32
    [B, G] with its mass on the selectable slots ([stop] scaled down so that walks last), uniforms from the same RandomState.  The host
    planner moves by SampledEpisode.sample; the kernel text draws from the same probabilities with its own inverse CDF.  Step by step:
    every table, the recorded action and the alive flag; at the end the ended flags and the number of live states."""
    import ndtw_cases
    from vln_goat_amd import rollout
    from vln_goat_amd.navdev import H
    scans, eps = ndtw_cases.case_two_scans()
    B, T = len(eps), 8
    sim, te = N.bench(scans, T)
    rs = np.random.RandomState(SAMPLE_SEED)
    u, probs, alive = rs.random_sample((T, B)), [], []

    def policy(t, p, part):
        sel = (part['s%d_gmap_masks' % t] & ~part['s%d_gmap_visited_masks' % t]).numpy()
        pr = rs.random_sample(sel.shape).astype(np.float32) * sel
        pr[:, 0] *= np.float32(0.05)
        probs.append(pr)
        alive.append(~p.ended)
        return np.where(p.ended, 0, rollout.SampledEpisode.sample(pr, N.FixedRng(u[t])))
    w = N.host_walk(te, eps, policy)
    assert w.stats['multi'] >= 1 and not w.ended[T - 2].all(), (w.stats, w.ended[T - 2])
    got = nav_cpu.cpu_walk(cpu_kernel, te, scans, eps, w, 'sample', probs=probs, u=u)
    assert np.array_equal(got.acts, np.asarray(w.acts)) and np.array_equal(got.alive, np.asarray(alive))
    assert N.check_sampling(probs, u, got.acts, got.alive) == int(np.sum(alive)) >= B + 1
    assert np.array_equal(got.blocks[:, H['ended']].astype(bool), w.p.ended) and int(got.blocks[:, H['live']].sum()) == w.p.n_traj
