"""EpisodePlanner(feedback='argmax') on the host (no GPU: the planner builds tables and walks the navigator only): the argmax stop
rule, the recorded stop scores, the backtrack to the best stop node, `pred_objid`, and the two older modes left as they were."""
import numpy as np
import pytest


def planner_case(reverie=False, T=5):
    from vln_goat_amd import rollout, synth
    if reverie:
        scan, feats, eps, dicts, objects = synth.make_reverie_rollout_case()
    else:
        scan, feats, eps, dicts = synth.make_rollout_case()
        objects = None
    rows = rollout._RowIndex(['%s_%s' % (scan.name, vp) for vp in scan.vpids])
    sim = rollout.GraphSim(rows, objects=objects.meta() if reverie else None, **({'obj_fallback': False} if reverie else {}))
    kw = dict(obj_width=6) if reverie else {}
    te = rollout.TeacherEpisode(sim, None, n_steps=T, text_len=32, pano_width=40, gmap_width=lambda t: 32, **kw)
    return te, eps


def first_fresh(p, i):
    """the first map slot of episode i that is a node not visited yet"""
    vp, visited = p._gin['gmap_vpids'][i], p._gin['gmap_visited_masks'][i]
    return next(a for a in range(1, len(vp)) if vp[a] is not None and not bool(visited[a]))


def test_argmax_walk_stops_records_scores_and_backtracks():
    from vln_goat_amd import rollout
    te, eps = planner_case()
    B = len(eps)
    p = rollout.EpisodePlanner(te, eps, imitation=False, feedback='argmax')
    visited = [[tr['path'][0][0]] for tr in p.traj]
    # episode 0 stops at once; episode 1 walks two nodes and stops with its best score at the FIRST node; episode 2 never stops (forced
    # end at the last step) with its best score at the node of step 2
    scores = np.array([[0.9, 0.8, 0.1], [0.0, 0.3, 0.2], [0.0, 0.5, 0.9], [0.0, 0.0, 0.3], [0.0, 0.0, 0.4]])
    for t in range(te.T):
        p.build_step()
        a = np.zeros(B, np.int64)
        if t < 2 and not p.ended[1]:
            a[1] = first_fresh(p, 1)
        if not p.ended[2]:
            a[2] = first_fresh(p, 2) if t < te.T - 1 else 3      # (the last step is a forced end whatever the action says)
        before = [ob['viewpoint'] for ob in p.obs]
        ended = p.ended.copy()
        p.advance(a, scores[t])
        for i in range(B):
            if not ended[i]:
                assert p.gmaps[i].node_stop_scores[before[i]] == {'stop': float(scores[t][i])}
                if before[i] != visited[i][-1]:
                    visited[i].append(before[i])
        if p.ended.all():
            break
    assert p.ended.all()
    tr = p.traj
    assert tr[0]['path'] == [[eps[0]['path'][0]]] and 'pred_objid' not in tr[0]
    # episode 1: two moves, then [stop] at step 2 (score 0.1) -> back to its start (score 0.8)
    flat1 = [vp for hop in tr[1]['path'] for vp in hop]
    assert len(visited[1]) == 3 and flat1[-1] == visited[1][0] and tr[1]['path'][-1][-1] == visited[1][0]
    assert [h[-1] for h in tr[1]['path'][:3]] == visited[1]
    # episode 2: walks to the last step; best score 0.9 at the node of step 2
    assert len(visited[2]) == te.T and tr[2]['path'][-1][-1] == visited[2][2]
    assert len(tr[2]['path']) == te.T + 1                          # start, T - 1 moves, the backtrack
    with pytest.raises(RuntimeError):
        p.advance(np.zeros(B, np.int64), scores[0])                # no step built


def test_argmax_walk_with_objects_sets_pred_objid():
    from vln_goat_amd import rollout
    te, eps = planner_case(reverie=True)
    B = len(eps)
    p = rollout.EpisodePlanner(te, eps, imitation=False, feedback='argmax')
    assert all(tr['pred_objid'] is None for tr in p.traj)
    p.build_step()
    with pytest.raises(ValueError):
        p.advance(np.zeros(B, np.int64), np.zeros(B))              # objects need the best-object row
    ids = [ob['obj_ids'] for ob in p.obs]
    best = np.array([max(len(x) - 1, 0) for x in ids], np.float32)
    p.advance(np.zeros(B, np.int64), np.full(B, 0.5, np.float32), best)
    assert p.ended.all()
    for i, tr in enumerate(p.traj):
        assert tr['pred_objid'] == (ids[i][int(best[i])] if len(ids[i]) > 0 else None)
        assert len(tr['path']) == 1


def test_older_modes_are_unchanged_and_bad_arguments_raise():
    from vln_goat_amd import rollout
    import torch
    te, eps = planner_case()
    with pytest.raises(ValueError):
        rollout.EpisodePlanner(te, eps, imitation=True, feedback='argmax')
    with pytest.raises(ValueError):
        rollout.EpisodePlanner(te, eps, imitation=False, feedback='sample')
    p = rollout.EpisodePlanner(te, eps, imitation=False, feedback='argmax')
    p.build_step()
    with pytest.raises(ValueError):
        p.advance(np.zeros(len(eps), np.int64))                    # an argmax walk needs the stop scores
    # teacher forcing: the stop rule is still the ground-truth goal, nothing is recorded, no backtrack
    a = te.plan(eps)
    q = rollout.EpisodePlanner(te, eps)
    for t in range(te.T):
        q.build_step()
        q.advance()
    b = q.finish()
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    assert all(not g.node_stop_scores for g in q.gmaps) and not hasattr(q, 'just_ended')
    for tr, ep in zip(q.traj, eps):
        assert [h[-1] for h in tr['path']] == ep['path'][:len(tr['path'])] and 'pred_objid' not in tr
