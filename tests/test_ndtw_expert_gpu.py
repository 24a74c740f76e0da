"""navdev.DeviceNavigator with the nDTW expert (goat_nav_ndtw, csrc/navexpert_core.hpp) against the host planner with
expert_policy='ndtw': after every step every `s{t}_*` tensor equals what EpisodePlanner.build_step() made for the same actions — the
labels by torch.equal — and trajectories, n_traj and the ended flags match (the comparison of test_device_navigator_gpu.py, kept in
ndtw_cases.py).  The preconditions are asserted on the host results first: the two experts disagree somewhere, several nodes are folded
in one step, a candidate lies three hops away, ordering by DTW is ordering by -nDTW in every labelled state.  Cases 1-3 and 5 need no model."""
import gc
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nav_cases as N
import ndtw_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda'


def _parity(scans, eps, T, policy, max_ref, gmap_width=None):
    from vln_goat_amd import rollout
    sim, te = N.bench(scans, T, gmap_width, expert_policy='ndtw')
    w = N.host_walk(te, eps, policy, observe=C.observe)
    bufs = rollout.EpisodeBuffers(te.plan(eps), device=DEV)
    tables = rollout.ScanTables(scans, sim.features, device=DEV)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'forced', max_ref=max_ref)
    assert nav.launches_per_step == 3
    return te, nav, bufs, w


def test_1_step_by_step_parity_two_scans():
    """scans of 24 (degree 3) and 29 (degree 2) nodes in one batch, B = 5, T = 8, forced mode under the host's random policy; ground-truth
    paths of exactly max_ref = 12, of 1 (start = goal) and of 2 viewpoints among them"""
    scans, eps = C.case_two_scans()
    te, nav, bufs, w = _parity(scans, eps, 8, N.random_policy(2, 0.05, scores=False), C.MAX_REF)
    C.preconditions(w.stats)
    N.same_walk(N.device_walk(nav, eps, bufs, w), w.p)


def test_2_more_candidates_than_a_wavefront():
    """one scan of 120 nodes, degree 6, B = 2, T = 20, the map bucket 128 wide: a step with more than 64 selectable unvisited nodes"""
    scans, eps = C.case_wide()
    te, nav, bufs, w = _parity(scans, eps, 20, C.frontier_policy, 24, gmap_width=lambda t: 128)
    C.preconditions(w.stats)
    assert w.stats['max_cands'] > 64, w.stats
    N.same_walk(N.device_walk(nav, eps, bufs, w), w.p)


def test_3_one_navigator_walks_two_batches():
    """the DTW row and the fold counter of the first walk do not leak into the second"""
    from vln_goat_amd import synth
    scans, eps = C.case_two_scans()
    te, nav, bufs, w = _parity(scans, eps, 8, N.random_policy(2, 0.05, scores=False), C.MAX_REF)
    N.same_walk(N.device_walk(nav, eps, bufs, w), w.p)
    rs = np.random.RandomState(77)
    e0 = synth.rxr_episodes(scans[0], rs, B=3, max_ref=C.MAX_REF, starts=[4, 13, 20])
    e1 = synth.rxr_episodes(scans[1], rs, B=2, max_ref=C.MAX_REF, starts=[5, 17])
    other = [e1[0], e0[0], e1[1], e0[1], e0[2]]
    for i, e in enumerate(other):
        e['instr_id'] = 'other%d' % i
    w2 = N.host_walk(te, other, N.random_policy(9, 0.05, scores=False), observe=C.observe)
    C.preconditions(w2.stats)
    N.same_walk(N.device_walk(nav, other, bufs, w2), w2.p)
    too_long = [dict(e) for e in other]
    too_long[3]['path'] = C.simple_path(scans[0], 0, C.MAX_REF + 1)
    with pytest.raises(ValueError, match='episode 3.*13 viewpoints'):
        nav.begin(too_long, actions=w2.acts)
    N.same_walk(N.device_walk(nav, eps, bufs, w), w.p)             # the refused batch launched nothing


# ---------------------------------------------------------------------------------------------------- with the model
def test_4_single_pass_end_to_end():
    """SinglePassSampledEpisode.run(navigator=) with the 'ndtw' navigator against the same object on the host planner
    (expert_policy='ndtw') under the same rng: equal actions and trajectories, the loss to 2e-5 (the bound
    test_device_navigator_gpu.test_e holds its two forms to)."""
    from vln_goat_amd import features, nav_model, rollout, synth
    scan, feats, _, dicts = synth.make_rollout_case()
    T, B = 5, 3
    eps = synth.rxr_episodes(scan, np.random.RandomState(7), B=B, max_ref=C.MAX_REF)      # (the experts disagree at step 0 already)
    torch.manual_seed(0)
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(SimpleNamespace(**N.EP_ARGS)))
    model.load_state_dict(synth.seeded_state_dict(model, seed=11))
    model = model.cuda().eval()
    store = features.FeatureStore.from_arrays({'%s_%s' % (scan.name, vp): feats[i] for i, vp in enumerate(scan.vpids)}, dtype=torch.float32).to('cuda')
    sim = rollout.GraphSim(store)
    call = lambda mode, batch: model(mode, batch)
    ex = synth.rollout_extras(dicts, B, 'cuda')
    te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=32, pano_width=40, expert_policy='ndtw')
    bufs = rollout.EpisodeBuffers(te.plan(eps))
    gc.collect()
    sp = rollout.SinglePassSampledEpisode(te, call, bufs, ex)
    tables = rollout.ScanTables([scan], store)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'sample', max_ref=C.MAX_REF)
    assert nav.launches_per_step == 3
    traj, actions = sp.run(eps, np.random.RandomState(100), navigator=nav)
    torch.cuda.synchronize()
    loss, n_traj = float(sp.loss), sp.n_traj
    ref_traj, ref_actions = sp.run(eps, np.random.RandomState(100))
    torch.cuda.synchronize()
    ref_loss = float(sp.loss)
    assert len(actions) == len(ref_actions) and all(np.array_equal(x, y) for x, y in zip(actions, ref_actions))
    assert [tr['path'] for tr in traj] == [tr['path'] for tr in ref_traj] and n_traj == sp.n_traj
    print('loss: device navigator %.7f, host planner %.7f' % (loss, ref_loss))
    assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    # the walk met a state the two experts label differently
    p = rollout.EpisodePlanner(te, eps, imitation=False)
    differ = 0
    for t in range(T):
        p.build_step()
        want, spl = C.planner_labels(p, 'ndtw'), C.planner_labels(p, 'spl')
        differ += int(((want != spl) & (want >= 0)).sum())
        p.advance(actions[t] if t < len(actions) else np.zeros(B, np.int64))
    assert differ >= 1


def test_5_spl_navigator_keeps_its_two_launches():
    from vln_goat_amd import rollout
    scans, eps = C.case_two_scans()
    sim, te = N.bench(scans, 4, expert_policy='spl')
    bufs = rollout.EpisodeBuffers(te.plan(eps), device=DEV)
    tables = rollout.ScanTables(scans, sim.features, device=DEV)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'forced')
    assert nav.launches_per_step == 2 and nav.expert == 'spl' and not hasattr(nav, 'xd')
