"""What the nDTW-expert tests share beside the bench of nav_cases.py (test_ndtw_expert.py on the CPU, test_ndtw_expert_gpu.py on the
device): the policies, what a host walk of EpisodePlanner(expert_policy='ndtw') records for the preconditions of the tests, and the
cases.  Nothing here needs a GPU."""
import numpy as np

MAX_REF = 12


def frontier_policy(t, p, part):
    """the selectable node with the most neighbours the map does not know yet: the map grows as fast as the scan lets it"""
    a = np.zeros(p.B, np.int64)
    vis = p._gin['gmap_visited_masks'].numpy()
    for b in range(p.B):
        if p.ended[b]:
            continue
        scan = p.obs[b]['scan_graph']
        known = set(p.gmaps[b].node_positions)
        best_n = -1
        for j, vp in enumerate(p._gin['gmap_vpids'][b]):
            if j > 1 and not vis[b][j]:
                n = sum(scan.vpids[k] not in known for k in scan.adj[scan.index[vp]])
                if n > best_n:
                    a[b], best_n = j, n
    return a


def planner_labels(p, expert_policy):
    """teacher_action of `expert_policy` on the state the planner's last build_step() saw"""
    from vln_goat_amd import nav_inputs
    return nav_inputs.teacher_action(p.obs, p._gin['gmap_vpids'], p.ended, p._gin['gmap_visited_masks'].numpy(), False, p.t, p.te.ignoreid,
                                     expert_policy=expert_policy, traj=p.traj)


def dtw_argmins(p):
    """per live episode off its goal: (the first strict minimum over -nDTW, the one over DTW, the candidates' hop counts), as
    teacher_action walks the slots"""
    from vln_goat_amd import nav_inputs
    out = []
    vis = p._gin['gmap_visited_masks'].numpy()
    for i, ob in enumerate(p.obs):
        if p.ended[i] or ob['viewpoint'] == ob['gt_path'][-1]:
            continue
        scan = ob['scan_graph']
        dist = scan.shortest()[0]
        walked = [scan.index[vp] for vp in sum(p.traj[i]['path'], [])]
        gt = [scan.index[vp] for vp in ob['gt_path']]
        best = {'n': (None, np.inf), 'd': (None, np.inf)}
        hops, first = [], True
        for j, vpid in enumerate(p._gin['gmap_vpids'][i]):
            if j > 1 and not vis[i][j]:
                there = [scan.index[vp] for vp in scan.shortest_path(ob['viewpoint'], vpid)[1:]]
                r = nav_inputs.cal_dtw(dist, walked + there, gt)
                hops.append(len(there))
                if -r['nDTW'] < best['n'][1]:
                    best['n'] = (j, -r['nDTW'])
                if first or r['DTW'] < best['d'][1]:
                    best['d'] = (j, r['DTW'])
                first = False
        out.append((best['n'][0], best['d'][0], hops))
    return out


def observe(t, p, part, stats):
    """nav_cases.host_walk(observe=): the step's labels are teacher_action of the planner's expert on its own state; counts labelled
    states, states whose 'ndtw' and 'spl' labels differ, the longest shortest path to a candidate, states where the order by -nDTW and
    the order by DTW disagree, the largest number of selectable unvisited nodes of a step"""
    for k in ('labelled', 'differ', 'max_hops', 'exp_disagrees', 'max_cands'):
        stats.setdefault(k, 0)
    want = planner_labels(p, p.te.expert_policy)
    assert np.array_equal(part['s%d_target' % t].numpy(), want)
    spl = planner_labels(p, 'spl')
    real = want >= 0
    stats['labelled'] += int(real.sum())
    stats['differ'] += int((want[real] != spl[real]).sum())
    for n_best, d_best, hops in dtw_argmins(p):
        stats['exp_disagrees'] += n_best != d_best
        stats['max_hops'] = max([stats['max_hops']] + hops)
        stats['max_cands'] = max(stats['max_cands'], len(hops))


def simple_path(scan, start, n):
    """a path of n distinct viewpoints from index `start` along the edges of the scan (depth first, neighbours in adjacency order)"""
    def grow(path):
        if len(path) == n:
            return path
        for j in scan.adj[path[-1]]:
            if j not in path:
                got = grow(path + [j])
                if got:
                    return got
        return None
    return [scan.vpids[i] for i in grow([start])]


def preconditions(stats, multi=True):
    """the host results make the parity meaningful: the two experts disagree somewhere, several nodes are folded in one step, a candidate
    lies three hops or more away, and ordering by DTW is ordering by -nDTW in EVERY labelled state"""
    assert stats['differ'] >= 1, stats
    if multi:
        assert stats['multi'] >= 1, stats
        assert stats['max_hops'] >= 3, stats
    assert stats['exp_disagrees'] == 0, stats


def case_two_scans(seed=21):
    """scans of 24 (degree 3) and 29 (degree 2) nodes in one batch, B = 5 (the shapes of test_device_navigator_gpu's case B), ground-truth
    paths of synth.rxr_episodes with three replaced by hand: exactly MAX_REF viewpoints, one viewpoint (start = goal), two viewpoints"""
    from vln_goat_amd import rollout, synth
    s0 = rollout.ScanGraph.synthetic('scanP', n=24, seed=3, degree=3)
    s1 = rollout.ScanGraph.synthetic('scanQ', n=29, seed=4, degree=2)
    rs = np.random.RandomState(seed)
    e0 = synth.rxr_episodes(s0, rs, B=3, max_ref=MAX_REF, starts=[1, 6, 11])
    e1 = synth.rxr_episodes(s1, rs, B=2, max_ref=MAX_REF, starts=[2, 9])
    eps = [e0[0], e1[0], e0[1], e1[1], e0[2]]
    eps[0]['path'] = simple_path(s0, s0.index[eps[0]['path'][0]], MAX_REF)
    eps[1]['path'] = eps[1]['path'][:1]
    eps[2]['path'] = simple_path(s0, s0.index[eps[2]['path'][0]], 2)
    for i, e in enumerate(eps):
        e['instr_id'] = 'ep%d' % i
    assert [len(e['path']) for e in eps][:3] == [MAX_REF, 1, 2] and all(2 < len(e['path']) <= MAX_REF for e in eps[3:])
    return [s0, s1], eps


def case_wide(seed=5, B=2):
    """one scan of 120 nodes, degree 6: more selectable unvisited nodes in a step than a wavefront has lanes"""
    from vln_goat_amd import rollout, synth
    scan = rollout.ScanGraph.synthetic('scanW', n=120, seed=7, degree=6)
    eps = synth.rxr_episodes(scan, np.random.RandomState(seed), B=B, max_ref=24, n_way=4, starts=[3, 50][:B])
    for i, e in enumerate(eps):
        e['instr_id'] = 'wide%d' % i
    return [scan], eps
