"""navdev.DeviceNavigator(objects=) (goat_nav_obj_step, csrc/navstate.hip) against the host planner with REVERIE objects: after every step
every `s{t}_*` tensor of the episode buffers, the ten object tables and all padding included, equals what EpisodePlanner.build_step()
made for the same actions; trajectories, n_traj, ended flags and `pred_objid` too.  The bounds are those of test_device_navigator_gpu.py:
torch.equal for every integer, bool, distance, label, scale, box and fusion value, 1e-6 absolute for the sin / cos / asin columns, which
now include the angle columns of the object rows of loc_fts.  The first four tests need no model; the last two run the captured walks
of test_argmax_walk_gpu.py's REVERIE case end to end."""
import gc

import numpy as np
import pytest
import torch

import nav_cases as N
import object_nav_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def case():
    """the bench of the CPU test on the device, and its two host walks (computed once, never written to)"""
    from vln_goat_amd import rollout
    scans, objects = C.scans_and_objects()
    eps = C.episodes(scans, objects)
    sim, te = C.bench(scans, objects)
    forced = N.host_walk(te, eps, C.policy(2), observe=C.observe)
    argmax = N.host_walk(te, eps, C.policy(2, tie=(1, (0, 1), 0.5)), 'argmax', C.observe)
    bufs = rollout.EpisodeBuffers(te.plan(eps), device=DEV)
    tables = rollout.ScanTables(scans, sim.features, device=DEV)
    ot = rollout.ObjectTables(objects, tables, device=DEV)
    return dict(scans=scans, objects=objects, eps=eps, te=te, forced=forced, argmax=argmax, bufs=bufs, tables=tables, ot=ot)


def _device_walk(te, eps, bufs, nav, mode, walk):
    """the navigator over `bufs` under the host walk's actions (and stop scores / best objects); every step's tables against the host's"""
    return N.device_walk(nav, eps, bufs, walk, mode, N.TABLES + N.OBJECT_TABLES)


def _same_walk(got, p, argmax):
    N.same_walk(got, p)
    traj = got[0]
    if argmax:
        assert [tr['pred_objid'] for tr in traj] == [tr['pred_objid'] for tr in p.traj]
    else:
        assert all('pred_objid' not in tr for tr in traj)


def test_forced_walk_builds_every_table_of_the_host_planner(case):
    from vln_goat_amd import rollout
    c = case
    C.preconditions(c['forced'].stats, c['forced'].ended)
    nav = rollout.DeviceNavigator(c['te'], c['tables'], c['bufs'], 'forced', objects=c['ot'], max_end=4)
    assert nav.launches_per_step == 2
    _same_walk(_device_walk(c['te'], c['eps'], c['bufs'], nav, 'forced', c['forced']), c['forced'].p, False)


def test_argmax_walk_records_the_best_objects_and_backtracks(case):
    from vln_goat_amd import rollout
    c = case
    w = c['argmax']
    parts, scores, bests, ended, p, stats = w.parts, w.scores, w.bests, w.ended, w.p, w.stats
    C.preconditions(stats, ended)
    # row 2 is negative wherever the viewpoint has no objects; episode 1 is scored twice with the same value on two viewpoints
    for t in range(c['te'].T):
        assert ((bests[t] < 0) == (parts[t]['s%d_reverie_obj_lens' % t].numpy() == 0)).all()
    assert scores[0][1] == scores[1][1] and not ended[0][1] and len(p.traj[1]['path']) >= 2
    want = [tr['pred_objid'] for tr in p.traj]
    assert any(x is None for x in want) and any(x is not None for x in want), want
    assert any(len(tr['path']) >= 3 and tr['path'][-1][-1] != tr['path'][-2][-1] for tr in p.traj)
    nav = rollout.DeviceNavigator(c['te'], c['tables'], c['bufs'], 'argmax', objects=c['ot'], max_end=4)
    _same_walk(_device_walk(c['te'], c['eps'], c['bufs'], nav, 'argmax', c['argmax']), p, True)


def test_a_second_walk_over_the_same_state_block_keeps_nothing_of_the_first(case):
    from vln_goat_amd import rollout
    c = case
    te = c['te']
    nav = rollout.DeviceNavigator(te, c['tables'], c['bufs'], 'argmax', objects=c['ot'], max_end=4)
    _same_walk(_device_walk(te, c['eps'], c['bufs'], nav, 'argmax', c['argmax']), c['argmax'].p, True)
    other = list(reversed(C.episodes(c['scans'], c['objects'], seed=5, absent=1)))
    for i, e in enumerate(other):
        e['instr_id'] = 'other%d' % i
    walk = N.host_walk(te, other, C.policy(7), 'argmax', C.observe)
    assert [tr['pred_objid'] for tr in walk.p.traj] != [tr['pred_objid'] for tr in c['argmax'].p.traj]
    _same_walk(_device_walk(te, other, c['bufs'], nav, 'argmax', walk), walk.p, True)
    goals = nav.goal.cpu().numpy()
    from vln_goat_amd import navdev
    assert np.array_equal(goals, navdev.object_goals(other, c['ot'], 4))


def test_a_viewpoint_with_more_objects_than_the_bucket_is_a_status_word(case):
    from vln_goat_amd import rollout
    c = case
    scans, objects, tables, ot = c['scans'], c['objects'], c['tables'], c['ot']
    sc = scans[0]
    count = {vp: len(ot.ids[tables.vp(sc.name, vp)]) for vp in sc.vpids}
    few = [vp for vp in sc.vpids if 1 <= count[vp] <= 3][0]
    none = [vp for vp in sc.vpids if count[vp] == 0][0]
    many = [vp for vp in sc.vpids if count[vp] == 5][0]
    ep = lambda i, vp: {'instr_id': 'w%d' % i, 'scan': sc, 'path': [vp], 'heading': 0.5 * i, 'instr_encoding': [1, 2, 3], 'end_vps': [vp],
                        'obj_id': ot.ids[tables.vp(sc.name, vp)][0] if count[vp] else None}
    ok, bad = [ep(0, few), ep(1, none)], [ep(0, few), ep(1, many)]
    sim, te = C.bench(scans, objects, T=2, obj_width=3)
    walk = N.host_walk(te, ok, C.policy(1), observe=C.observe)
    assert walk.stats['labelled'] >= 1
    bufs = rollout.EpisodeBuffers(te.plan(ok), device=DEV)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'forced', objects=ot, max_end=2)
    nav.begin(bad, actions=walk.acts)
    for t in range(te.T + 1):
        nav.step(t)
    with pytest.raises(ValueError, match=r'episode 1, step 0.*objects'):
        nav.finish()
    _same_walk(_device_walk(te, ok, bufs, nav, 'forced', walk), walk.p, False)


# ---------------------------------------------------------------------------------------------------- with the model
def test_argmax_episode_runs_on_the_object_navigator():
    """ArgmaxEpisode.run(navigator=) on synth.make_reverie_rollout_case() with the model of test_argmax_walk_gpu.py's reverie case: paths,
    pred_objid and recorded actions equal walk.run(episodes) on the host planner, also with check_every=1"""
    import test_argmax_walk_gpu as AW
    from vln_goat_amd import rollout
    c = AW.build(True)
    te, bufs = c['te'], c['bufs']
    walk = rollout.ArgmaxEpisode(te, c['model'], bufs, c['ex'])
    tables = rollout.ScanTables([c['scan']], c['store'])
    ot = rollout.ObjectTables(te.objects, tables)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'argmax', objects=ot, max_end=4)
    found = 0
    for episodes in (c['eps'], c['other'], c['eps']):
        traj = walk.run(episodes, navigator=nav)
        actions = [a.copy() for a in walk.actions]
        assert N.masks_match() > 0
        early = walk.run(episodes, navigator=nav, check_every=1)
        assert early == traj
        assert len(walk.actions) == len(actions) and all(np.array_equal(x, y) for x, y in zip(walk.actions, actions))
        ref = walk.run(episodes)
        assert all(np.array_equal(x, y) for x, y in zip(walk.actions, actions[:len(walk.actions)]))
        assert [tr['path'] for tr in traj] == [tr['path'] for tr in ref]
        assert [tr['pred_objid'] for tr in traj] == [tr['pred_objid'] for tr in ref]
        found += sum(tr['pred_objid'] is not None for tr in traj)
    assert found >= 1


def test_single_pass_sampled_episode_runs_on_the_object_navigator():
    """SinglePassSampledEpisode.run(navigator=) on the same case: the recorded actions are SampledEpisode.sample of the live
    probabilities; the host path under those actions gives the same trajectories, the same loss (2e-5) and the same parameter gradients
    (5e-4 of their scale): the bounds of test_device_navigator_gpu.py's case E, which hold the host single pass to the eager one."""
    import test_argmax_walk_gpu as AW
    from vln_goat_amd import rollout
    c = AW.build(True)
    te, bufs, model = c['te'], c['bufs'], c['model']
    params = [p for p in model.parameters()]
    names = {id(p): n for n, p in model.named_parameters()}
    T, B = te.T, len(c['eps'])
    gc.collect()
    sp = rollout.SinglePassSampledEpisode(te, lambda mode, batch: model(mode, batch), bufs, c['ex'])
    tables = rollout.ScanTables([c['scan']], c['store'])
    nav = rollout.DeviceNavigator(te, tables, bufs, 'sample', objects=rollout.ObjectTables(te.objects, tables), max_end=4)

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
    for rnd, episodes in enumerate((c['eps'], c['other'])):
        zero()
        u = np.random.RandomState(100 + rnd).random_sample((T, B))
        traj, actions = sp.run(episodes, np.random.RandomState(100 + rnd), navigator=nav)
        torch.cuda.synchronize()
        assert N.masks_match() > 0
        probs = [pr.float().cpu().numpy() for pr in sp.probs]
        assert N.check_sampling(probs[:len(actions)], u, actions, nav.alive) >= B
        loss = float(sp.loss)
        grads = {id(p): (None if p.grad is None else p.grad.detach().clone()) for p in params}
        n_traj = sp.n_traj
        zero()
        ref_traj, ref_actions = sp.run(episodes, sampler=lambda t, pr: actions[t])
        torch.cuda.synchronize()
        assert [tr['path'] for tr in traj] == [tr['path'] for tr in ref_traj]
        assert len(actions) == len(ref_actions) and all(np.array_equal(x, y) for x, y in zip(actions, ref_actions))
        assert n_traj == sp.n_traj
        ref_loss = float(sp.loss)
        print('round %d: loss %.7f against %.7f' % (rnd, loss, ref_loss))
        assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (rnd, loss, ref_loss)
        top = max(float(p.grad.abs().max()) for p in params if p.grad is not None)
        n = 0
        for p in params:
            if p.grad is None:
                assert grads[id(p)] is None, names[id(p)]
                continue
            scale = max(float(p.grad.abs().max()), 1e-3 * top)
            err = float((grads[id(p)] - p.grad).abs().max())
            assert err <= 5e-4 * scale, (rnd, names[id(p)], err, scale)
            n += 1
        assert n > 100
