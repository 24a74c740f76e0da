"""What the object-navigator tests share beside the bench of nav_cases.py (test_object_navigator.py on the CPU,
test_object_navigator_gpu.py on the device): the REVERIE case over two scans, its policy, and what a host walk of EpisodePlanner with
objects records for the tests' preconditions.  Nothing here needs a GPU."""
import numpy as np
import torch

import nav_cases as N

T, B, O, W = 6, 6, 5, 40
ABSENT = 10 ** 6          # an object id no viewpoint holds


def scans_and_objects():
    from vln_goat_amd import rollout
    scans = [rollout.ScanGraph.synthetic('scanP', n=22, seed=3, degree=3), rollout.ScanGraph.synthetic('scanQ', n=17, seed=4, degree=2)]
    objects = rollout.ObjectStore.synthetic(scans, max_objects=5, seed=22, dtype=torch.float32, p_empty=0.2)
    return scans, objects


def bench(scans, objects, T=T, obj_width=O, obj_fallback=False):
    """nav_cases.bench with the objects' metadata in the simulator"""
    return N.bench(scans, T, objects=objects.meta(), obj_fallback=obj_fallback, W=W, obj_width=obj_width)


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


def observe(t, p, part, stats):
    """nav_cases.host_walk(observe=): live states on a viewpoint without objects / with a full bucket, labelled object targets, live
    states on an end viewpoint whose target is absent"""
    for k in ('no_objects', 'full_bucket', 'labelled', 'absent_on_goal'):
        stats.setdefault(k, 0)
    live = ~p.ended
    olens = part['s%d_reverie_obj_lens' % t].numpy()
    otgt = part['s%d_obj_target' % t].numpy()
    stats['no_objects'] += int((live & (olens == 0)).sum())
    stats['full_bucket'] += int((live & (olens == p.te.O)).sum())
    stats['labelled'] += int((otgt != p.te.ignoreid).sum())
    for i, ob in enumerate(p.obs):
        stats['absent_on_goal'] += int(live[i] and ob['viewpoint'] in ob['gt_end_vps'] and otgt[i] == p.te.ignoreid)


def preconditions(stats, ended, T=T):
    """the host walk makes the parity meaningful: a live state on a viewpoint without objects and one with a full bucket, a labelled
    object target, an end viewpoint whose target is absent, a multi-hop move, an averaged node, and someone still walking at T - 1"""
    for k in ('no_objects', 'full_bucket', 'labelled', 'multi', 'absent_on_goal', 'avg'):
        assert stats[k] >= 1, stats
    assert not ended[T - 2].all(), 'no episode alive at T - 1'
