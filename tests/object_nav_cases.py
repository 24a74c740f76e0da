"""What the object-navigator tests share (test_object_navigator.py on the CPU, test_object_navigator_gpu.py on the device): the REVERIE
bench over two scans, the host walk of EpisodePlanner with objects that records what the tests' preconditions need, and the table
comparison of test_device_navigator_gpu.py widened by the ten object tables.  Nothing here needs a GPU."""
import numpy as np
import torch

A = 4
TABLES = ('feat_idx', 'feat_start', 'loc_fts', 'nav_types', 'view_lens', 'gmap_step_ids', 'gmap_pos_fts', 'gmap_pair_dists', 'gmap_visited_masks',
          'gmap_masks', 'vp_pos_fts', 'vp_masks', 'vp_nav_masks', 'nav_fusion', 'target', 'csr_idx', 'csr_start', 'csr_scale', 'inv_idx', 'inv_start',
          'inv_w')
OBJECT_TABLES = ('obj_idx', 'obj_start', 'reverie_obj_lens', 'reverie_obj_names', 'vp_obj_masks', 'obj_target', 'ocat_idx', 'ocat_start',
                 'ocat_inv_idx', 'ocat_inv_start')
# columns that go through sin / cos / asin (and the line distance): 1e-6; every other column exact (test_device_navigator_gpu.py).  The
# angle columns of loc_fts now include those of the object rows.
LOOSE = {'loc_fts': list(range(A)), 'gmap_pos_fts': list(range(A + 1)), 'vp_pos_fts': list(range(A + 1)) + [A + 3 + c for c in range(A + 1)]}
T, B, O, W = 6, 6, 5, 40
ABSENT = 10 ** 6          # an object id no viewpoint holds


def scans_and_objects():
    from vln_goat_amd import rollout
    scans = [rollout.ScanGraph.synthetic('scanP', n=22, seed=3, degree=3), rollout.ScanGraph.synthetic('scanQ', n=17, seed=4, degree=2)]
    objects = rollout.ObjectStore.synthetic(scans, max_objects=5, seed=22, dtype=torch.float32, p_empty=0.2)
    return scans, objects


def bench(scans, objects, T=T, obj_width=O, obj_fallback=False):
    """sim over a key -> row index of `scans` with the objects' metadata, and the episode bucket"""
    from vln_goat_amd import rollout
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    sim = rollout.GraphSim(rollout._RowIndex(keys), objects=objects.meta(), obj_fallback=obj_fallback)
    te = rollout.TeacherEpisode(sim, None, n_steps=T, text_len=32, pano_width=W, obj_width=obj_width)
    return sim, te


def episodes(scans, objects, seed=21, B=B, T=T, absent=2):
    """synth.reverie_episodes of the two scans interleaved as test_device_navigator_gpu._two_scans does; episode `absent` asks for an
    object no viewpoint holds"""
    from vln_goat_amd import synth
    s0, s1 = scans
    n0, n1 = len(s0.vpids), len(s1.vpids)
    rs = np.random.RandomState(seed)
    e0 = synth.reverie_episodes(s0, objects, rs, B=(B + 1) // 2, max_steps=T, starts=[(5 * b + 1) % n0 for b in range((B + 1) // 2)])
    e1 = synth.reverie_episodes(s1, objects, rs, B=B // 2, max_steps=T, starts=[(7 * b + 2) % n1 for b in range(B // 2)])
    eps = [e for pair in zip(e0, e1) for e in pair] + e0[len(e1):]
    for i, e in enumerate(eps):
        e['instr_id'] = 'ep%d' % i
    if absent is not None:
        eps[absent]['obj_id'] = ABSENT
    return eps


def policy(seed, p_stop=0.05, tie=None):
    """even episodes follow the step's `target` label, odd ones pick a random selectable node or, with p_stop, stop.  -> (actions,
    stop scores, best objects): the best object is a random one of the viewpoint's, and a negative number where it has none (what
    ArgmaxEpisode leaves there); tie = (episode, steps, score): equal stop scores for that episode at those steps."""
    rs = np.random.RandomState(seed)

    def pick(t, p, part):
        sel = (part['s%d_gmap_masks' % t] & ~part['s%d_gmap_visited_masks' % t]).numpy()
        target = part['s%d_target' % t].numpy()
        olens = part['s%d_reverie_obj_lens' % t].numpy()
        vlens = part['s%d_view_lens' % t].numpy()
        a = np.zeros(p.B, np.int64)
        for b in range(p.B):
            stop = rs.uniform() < p_stop
            slots = np.nonzero(sel[b, 2:])[0] + 2
            rand = int(slots[rs.randint(len(slots))]) if len(slots) else 0
            if p.ended[b]:
                a[b] = 0
            elif b % 2 == 0:
                a[b] = max(int(target[b]), 0)
            else:
                a[b] = 0 if stop else rand
        scores = rs.uniform(0.05, 0.95, p.B).astype(np.float32)
        if tie is not None and t in tie[1]:
            scores[tie[0]] = np.float32(tie[2])
        best = np.array([rs.randint(n) if n else -(int(v) + 2) for n, v in zip(olens, vlens)], np.float32)
        return a, scores, best
    return pick


def host_walk(te, eps, pick, feedback=None):
    """EpisodePlanner(te) with objects driven by pick(t, planner, part) -> per-step tables, actions, stop scores, best objects, ended flags
    after every move, the planner and the counts the preconditions ask for"""
    from vln_goat_amd import rollout
    p = rollout.EpisodePlanner(te, eps, imitation=False, feedback=feedback)
    parts, acts, scores, bests, ended = [], [], [], [], []
    stats = {'no_objects': 0, 'full_bucket': 0, 'labelled': 0, 'multi': 0, 'absent_on_goal': 0, 'avg': 0}
    for t in range(te.T):
        part = {k: v.clone() for k, v in p.build_step().items()}
        live = ~p.ended
        olens = part['s%d_reverie_obj_lens' % t].numpy()
        otgt = part['s%d_obj_target' % t].numpy()
        stats['no_objects'] += int((live & (olens == 0)).sum())
        stats['full_bucket'] += int((live & (olens == te.O)).sum())
        stats['labelled'] += int((otgt != te.ignoreid).sum())
        stats['avg'] += int((part['s%d_csr_scale' % t] < 1).sum())
        for i, ob in enumerate(p.obs):
            stats['absent_on_goal'] += int(live[i] and ob['viewpoint'] in ob['gt_end_vps'] and otgt[i] == te.ignoreid)
        a, s, o = pick(t, p, part)
        before = [len(tr['path']) for tr in p.traj]
        if feedback == 'argmax':
            p.advance(a, s, o)
        else:
            p.advance(a)
        for tr, n in zip(p.traj, before):
            stats['multi'] += sum(len(hop) > 1 for hop in tr['path'][n:n + 1])
        parts.append(part)
        acts.append(np.asarray(a, np.int64))
        scores.append(np.asarray(s, np.float32))
        bests.append(np.asarray(o, np.float32))
        ended.append(p.ended.copy())
    return parts, acts, scores, bests, ended, p, stats


def preconditions(stats, ended, T=T):
    """the host walk makes the parity meaningful: a live state on a viewpoint without objects and one with a full bucket, a labelled
    object target, an end viewpoint whose target is absent, a multi-hop move, an averaged node, and someone still walking at T - 1"""
    for k in ('no_objects', 'full_bucket', 'labelled', 'multi', 'absent_on_goal', 'avg'):
        assert stats[k] >= 1, stats
    assert not ended[T - 2].all(), 'no episode alive at T - 1'


def compare(t, got, want, tables=TABLES + OBJECT_TABLES):
    """every table of step t, padding included (got: {key: tensor} on any device)"""
    for name in tables:
        k = 's%d_%s' % (t, name)
        g, w = got[k].cpu(), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if name in LOOSE:
            loose = torch.zeros(g.shape[-1], dtype=torch.bool)
            loose[LOOSE[name]] = True
            assert torch.equal(g[..., ~loose], w[..., ~loose]), k
            err = float((g[..., loose] - w[..., loose]).abs().max())
            assert err <= 1e-6, (k, err)
        else:
            assert torch.equal(g, w), (k, g.reshape(-1)[:48], w.reshape(-1)[:48])
