"""navdev.DeviceNavigator (csrc/navstate.hip) against the host planner it restates: after every step every `s{t}_*` tensor of the episode
buffers, padding included, equals what EpisodePlanner.build_step() made for the same actions; trajectories, n_traj and the ended flags
too.  Integer, bool and distance tables, labels, scales and the fusion matrix are compared with torch.equal; the sin / cos / asin columns
(and the line distance behind an asin-free sqrt that shares their column block) to 1e-6 absolute: values of magnitude <= 1 from another
math library, 1e-6 being about 16 float32 ulps at 1.0.  Cases A-D need no model; E and F run the captured walks end to end."""
import gc
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nav_cases as N

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda'


def _navigator(te, scans, eps, sim, mode='forced'):
    from vln_goat_amd import rollout
    bufs = rollout.EpisodeBuffers(te.plan(eps), device=DEV)
    tables = rollout.ScanTables(scans, sim.features, device=DEV)
    return rollout.DeviceNavigator(te, tables, bufs, mode), bufs


def _parity(scans, eps, T, seed, p_stop, mode='forced', gmap_width=None):
    sim, te = N.bench(scans, T, gmap_width)
    w = N.host_walk(te, eps, N.random_policy(seed, p_stop), 'argmax' if mode == 'argmax' else None)
    nav, bufs = _navigator(te, scans, eps, sim, mode)
    N.same_walk(N.device_walk(nav, eps, bufs, w, mode), w.p)
    return w.stats, w.ended


def _conditions(stats, ended, T, multi=True):
    if multi:
        assert stats['multi'] >= 1, stats
    assert stats['avg'] >= 1, stats
    assert not ended[T - 2].all(), 'no episode alive at T - 1'
    assert ended[1].sum() <= len(ended[1]) // 2, 'more than half of the episodes ended before step 2'


def _two_scans(n0, d0, n1, d1, B, T, seed):
    from vln_goat_amd import rollout, synth
    s0 = rollout.ScanGraph.synthetic('scanP', n=n0, seed=3, degree=d0)
    s1 = rollout.ScanGraph.synthetic('scanQ', n=n1, seed=4, degree=d1)
    rs = np.random.RandomState(seed)
    e0 = synth.rollout_episodes(s0, rs, B=(B + 1) // 2, max_steps=T, starts=[(5 * b + 1) % n0 for b in range((B + 1) // 2)])
    e1 = synth.rollout_episodes(s1, rs, B=B // 2, max_steps=T, starts=[(7 * b + 2) % n1 for b in range(B // 2)])
    eps = [e for pair in zip(e0, e1) for e in pair] + e0[len(e1):]
    for i, e in enumerate(eps):
        e['instr_id'] = 'ep%d' % i
    return [s0, s1], eps


def test_case_a_fixture_actions():
    """A: synth.make_rollout_case() (24 nodes, B = 3, T = 5) under the sampled actions of the reference's own rollout."""
    from vln_goat_amd import synth
    z = np.load(os.path.join(HERE, 'golden', 'rollout_episode_sample.npz'))
    scan, _, eps, _ = synth.make_rollout_case()
    T = int(z['n_steps'][0])
    sim, te = N.bench([scan], T)
    w = N.host_walk(te, eps, lambda t, p, part: np.where(p.ended, 0, z['s%d_action' % t]))
    assert w.stats['avg'] >= 1 and not w.ended[T - 2].all()
    nav, bufs = _navigator(te, [scan], eps, sim)
    N.same_walk(N.device_walk(nav, eps, bufs, w), w.p)


def test_case_b_two_scans_in_one_batch():
    """B: scans of 24 (degree 3) and 29 (degree 2) nodes in one batch, B = 5, T = 8: multi-hop moves, averaged nodes, map rows with
    several fusion entries, ends forced at T - 1."""
    scans, eps = _two_scans(24, 3, 29, 2, 5, 8, seed=21)
    stats, ended = _parity(scans, eps, 8, seed=2, p_stop=0.05)
    _conditions(stats, ended, 8)
    assert stats['fusion_rows'] >= 1, stats


def test_case_c_argmax_stop_scores_and_backtrack():
    """C: argmax mode on a 4-node scan, B = 2, T = 6.  Episode 0 never stops: every node gets visited and no_vp_left ends it; episode 1
    stops at step 0.  Equal stop scores: the first maximum in visit order is the backtrack's node."""
    from vln_goat_amd import rollout, synth
    scan = rollout.ScanGraph.synthetic('scanC', n=4, seed=1, degree=1)
    T = 6
    eps = synth.rollout_episodes(scan, np.random.RandomState(3), B=2, max_steps=T, starts=[0, 2])
    sim, te = N.bench([scan], T)
    tie = np.float32(0.5)

    def policy(t, p, part):
        sel = (part['s%d_gmap_masks' % t] & ~part['s%d_gmap_visited_masks' % t]).numpy()
        slots = np.nonzero(sel[0, 2:])[0] + 2
        a0 = int(slots[0]) if len(slots) and not p.ended[0] else 0
        # episode 0: a tie between its first two nodes, lower scores behind them; episode 1 stops at once
        return np.array([a0, 0], np.int64), np.array([tie if t < 2 else 0.25, 0.75], np.float32)
    w = N.host_walk(te, eps, policy, 'argmax')
    p, ended = w.p, w.ended
    assert w.stats['noleft'] >= 1 and ended[0][1] and not ended[0][0], (w.stats, ended)
    start0 = eps[0]['path'][0]
    assert p.traj[0]['path'][-1][-1] == start0 and len(p.traj[0]['path']) >= 3, p.traj[0]      # back to the FIRST of the tied nodes
    nav, bufs = _navigator(te, [scan], eps, sim, 'argmax')
    got = N.device_walk(nav, eps, bufs, w, 'argmax')
    N.same_walk(got, p)
    assert all(np.array_equal(x, y) for x, y in zip(got[1], w.acts[:len(got[1])]))


def test_case_d_full_bucket():
    """D: B = 12, T = 15 on scans of 40 and 45 nodes with the default 128-wide last bucket."""
    scans, eps = _two_scans(40, 3, 45, 3, 12, 15, seed=8)
    stats, ended = _parity(scans, eps, 15, seed=5, p_stop=0.05)
    _conditions(stats, ended, 15)


def test_sampling_is_the_hosts():
    """sample mode over synthetic probabilities written where the step graphs would leave them: zero-mass padding slots, a row whose
    mass sits in its last real slot, uniforms next to 1.  Exact equality with SampledEpisode.sample."""
    from vln_goat_amd import rollout, synth
    scan = rollout.ScanGraph.synthetic('scanS', n=24, seed=9, degree=3)
    T, B = 4, 4
    eps = synth.rollout_episodes(scan, np.random.RandomState(1), B=B, max_steps=T, starts=[0, 5, 9, 14])
    sim, te = N.bench([scan], T)
    nav, bufs = _navigator(te, [scan], eps, sim, 'sample')
    rs = np.random.RandomState(4)
    u = rs.random_sample((T, B))
    u[:, 1] = 1.0 - 2.0 ** -53          # the largest double below 1
    u[0, 2] = 0.0
    nav.begin(eps, N.FixedRng(u))
    probs = []
    for t in range(T + 1):
        if t > 0:
            # probabilities over the selectable slots of step t - 1 as the navigator left them; [stop] never: every episode walks on
            sel = (bufs.t['s%d_gmap_masks' % (t - 1)] & ~bufs.t['s%d_gmap_visited_masks' % (t - 1)]).cpu().numpy()
            sel[:, :2] = False
            p = rs.uniform(0.01, 1.0, sel.shape).astype(np.float32) * sel
            last = np.nonzero(sel[3])[0]
            if len(last):
                p[3] = 0
                p[3, last[-1]] = 0.7          # the whole mass in the last real slot
            p = (p / np.maximum(p.sum(1, keepdims=True), 1e-30)).astype(np.float32)
            probs.append(p)
            nav.step(t, torch.from_numpy(p).to(DEV))
        else:
            nav.step(0)
        torch.cuda.synchronize()
    traj, actions, n_traj, ended = nav.finish()
    assert len(actions) == T
    assert N.check_sampling(probs, u, actions, nav.alive) >= B * (T - 1)
    for t in range(T - 1):                  # no padding slot, no visited node was drawn: the walk took a hop at every step but the last
        assert all(len(tr['path']) == T for tr in traj), [len(tr['path']) for tr in traj]


def _status_bench():
    from vln_goat_amd import rollout, synth
    scan = rollout.ScanGraph.synthetic('scanE', n=24, seed=9, degree=3)
    T, B = 4, 2
    eps = synth.rollout_episodes(scan, np.random.RandomState(1), B=B, max_steps=T, starts=[0, 5])
    return scan, T, B, eps


def test_status_words_raise_and_the_process_stays_usable():
    from vln_goat_amd import rollout
    scan, T, B, eps = _status_bench()
    sim, te = N.bench([scan], T)
    w = N.host_walk(te, eps, N.random_policy(3, 0.0))
    acts, p = w.acts, w.p
    nav, bufs = _navigator(te, [scan], eps, sim)
    bad = [a.copy() for a in acts]
    bad[1][1] = 2                       # slot 2 of step 1 is the start node: visited
    nav.begin(eps, actions=bad)
    for t in range(T + 1):
        nav.step(t)
    with pytest.raises(ValueError, match=r'episode 1, step 1'):
        nav.finish()
    traj, _, n_traj, _ = N.device_walk(nav, eps, bufs, w)       # a second, valid walk over the same state block
    assert [tr['path'] for tr in traj] == [tr['path'] for tr in p.traj] and n_traj == p.n_traj
    # a bucket narrower than the map
    # (buffers of that width from a 4-node scan, whose maps fit; the 24-node scan's do not)
    from vln_goat_amd import synth
    small = rollout.ScanGraph.synthetic('scanC', n=4, seed=1, degree=1)
    eps4 = synth.rollout_episodes(small, np.random.RandomState(3), B=B, max_steps=T, starts=[0, 2])
    sim8, te8 = N.bench([scan, small], T, gmap_width=lambda t: 8)
    nav8, bufs8 = _navigator(te8, [scan, small], eps4, sim8)
    nav8.begin(eps, actions=acts)
    for t in range(T + 1):
        nav8.step(t)
    with pytest.raises(ValueError, match=r'episode \d, step \d.*map'):
        nav8.finish()
    w4 = N.host_walk(te8, eps4, N.random_policy(4, 0.0))
    p4 = w4.p
    traj, _, n_traj, _ = N.device_walk(nav8, eps4, bufs8, w4)
    assert [tr['path'] for tr in traj] == [tr['path'] for tr in p4.traj] and n_traj == p4.n_traj


# ---------------------------------------------------------------------------------------------------- with the model (E, F, masks)
def _model():
    from vln_goat_amd import nav_model, synth
    cfg = nav_model.nav_config_from_args(SimpleNamespace(**N.EP_ARGS))
    torch.manual_seed(0)
    m = nav_model.GlocalTextPathNavCMT(cfg)
    m.load_state_dict(synth.seeded_state_dict(m, seed=11))
    return m.cuda().eval()


def _store(scan, feats, dtype):
    from vln_goat_amd import features
    return features.FeatureStore.from_arrays({'%s_%s' % (scan.name, vp): feats[i] for i, vp in enumerate(scan.vpids)}, dtype=dtype).to('cuda')


def test_e_single_pass_end_to_end_and_mask_memo():
    """E: SinglePassSampledEpisode.run(navigator=) on eps, other, eps again: the recorded actions are SampledEpisode.sample of the
    live probabilities; the same object on the host path under those actions gives the same trajectories, the same loss (2e-5) and the
    same parameter gradients (5e-4 of their scale) — the bounds the host single pass is held to against the eager one.  After every
    walk every memoised mask equals its recomputation (two walks over the same buffers with different episodes)."""
    from vln_goat_amd import rollout, synth
    z = np.load(os.path.join(HERE, 'golden', 'rollout_episode_sample.npz'))
    scan, feats, eps, dicts = synth.make_rollout_case()
    model = _model()
    store = _store(scan, feats, torch.float32)
    sim = rollout.GraphSim(store)
    call = lambda mode, batch: model(mode, batch)
    ex = synth.rollout_extras(dicts, len(eps), 'cuda')
    T = int(z['n_steps'][0])
    params = [p for p in model.parameters()]
    names = {id(p): n for n, p in model.named_parameters()}
    te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=32, pano_width=40)
    bufs = rollout.EpisodeBuffers(te.plan(eps))
    gc.collect()
    sp = rollout.SinglePassSampledEpisode(te, call, bufs, ex)
    tables = rollout.ScanTables([scan], store)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'sample')
    other = synth.rollout_episodes(scan, np.random.RandomState(5), B=3, max_steps=4, starts=[3, 11, 16])

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
    for rnd, episodes in enumerate((eps, other, eps)):
        zero()
        u = np.random.RandomState(100 + rnd).random_sample((T, len(eps)))
        traj, actions = sp.run(episodes, np.random.RandomState(100 + rnd), navigator=nav)
        torch.cuda.synchronize()
        assert N.masks_match() > 0
        probs = [pr.float().cpu().numpy() for pr in sp.probs]
        assert N.check_sampling(probs, u, [a for a in actions] + [None] * (T - len(actions)), nav.alive) >= len(eps)
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
        assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (rnd, loss, ref_loss)
        top = max(float(p.grad.abs().max()) for p in params if p.grad is not None)
        n = 0
        for p in params:
            if p.grad is None:
                assert grads[id(p)] is None, names[id(p)]
                continue
            scale = max(float(p.grad.abs().max()), 1e-3 * top)
            assert float((grads[id(p)] - p.grad).abs().max()) <= 5e-4 * scale, (rnd, names[id(p)], float((grads[id(p)] - p.grad).abs().max()), scale)
            n += 1
        assert n > 100


def test_f_argmax_walk_end_to_end():
    """F: ArgmaxEpisode.run(navigator=): the trajectories equal the host planner (feedback='argmax') advanced with the actions and stop
    scores the device walk recorded, and the host walk of the same object."""
    from vln_goat_amd import rollout, synth
    scan, feats, eps, dicts = synth.make_rollout_case()
    model = _model()
    store = _store(scan, feats, torch.float32)
    sim = rollout.GraphSim(store)
    call = lambda mode, batch: model(mode, batch)
    ex = synth.rollout_extras(dicts, len(eps), 'cuda')
    T = 5
    te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=32, pano_width=40)
    bufs = rollout.EpisodeBuffers(te.plan(eps))
    walk = rollout.ArgmaxEpisode(te, call, bufs, ex)
    tables = rollout.ScanTables([scan], store)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'argmax')
    other = synth.rollout_episodes(scan, np.random.RandomState(5), B=3, max_steps=4, starts=[3, 11, 16])
    for episodes in (eps, other, eps):
        traj = walk.run(episodes, navigator=nav)
        actions = [a.copy() for a in walk.actions]
        assert N.masks_match() > 0
        scores = nav.sd.view(len(eps), -1)[:, nav.cap * nav.cap:].cpu().numpy()
        early = walk.run(episodes, navigator=nav, check_every=1)          # the host stops replaying once nobody walks
        assert [tr['path'] for tr in early] == [tr['path'] for tr in traj]
        assert len(walk.actions) == len(actions) and all(np.array_equal(x, y) for x, y in zip(walk.actions, actions))
        ref = walk.run(episodes)
        assert all(np.array_equal(x, y) for x, y in zip(walk.actions, actions[:len(walk.actions)]))
        assert [tr['path'] for tr in traj] == [tr['path'] for tr in ref]
        # the host planner under the device's recorded actions and stop scores
        p = rollout.EpisodePlanner(te, episodes, imitation=False, feedback='argmax')
        for t in range(T):
            p.build_step()
            s = np.zeros(len(eps), np.float32)
            for b in range(len(eps)):
                if not p.ended[b]:
                    node = list(p.gmaps[b].node_positions).index(p.obs[b]['viewpoint'])
                    s[b] = scores[b, node]
            p.advance(actions[t] if t < len(actions) else np.zeros(len(eps), np.int64), s, None)
        assert [tr['path'] for tr in traj] == [tr['path'] for tr in p.traj]
