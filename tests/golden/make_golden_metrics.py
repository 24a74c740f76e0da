"""Golden vectors for the validation metrics FROM THE IMPORTED REFERENCE (this container only):

  * `R2RNavBatch._eval_item` / `eval_metrics` of the reference's map_nav_src/r2r/env.py:452-520 (with `cal_dtw` / `cal_cls` of
    r2r/eval_utils.py) and `ReverieObjectNavBatch._eval_item` / `eval_metrics` of reverie/env.py:530-581, called as plain functions on a
    stand-in `self` that holds `shortest_distances`, `gt_trajs` and `obj2vps` only.  Both modules import MatterSim and half a dozen
    packages this image lacks; they are replaced by EMPTY modules for the import — none of their attributes is used by the four functions.
  * the distance tables are built as the reference builds them (utils/data.py:76-101 + r2r/env.py:183-189): an `nx.Graph` whose edge
    weights are the Euclidean distances of the poses, then `nx.all_pairs_dijkstra_path_length`.

Content: three synthetic scans (12 nodes on an integer grid with 3.0-long edges, so that some nav_error is EXACTLY the 3.0 margin; 33
and 60 random nodes), items of every (P, R) in PR below with repeated nodes in the predicted paths, scans interleaved; the REVERIE items
carry goal sets of 1 and 4 viewpoints with the last node inside and outside the set.

The script also evaluates a numpy restatement of the summed columns (3 trajectory_lengths, 4 gt_lengths, 7 spl, 9 nDTW, 10 SDTW, 11 CLS)
with the summation order REVERSED and records the largest relative deviation from the reference in the json: it must stay below 1e-13,
a tenth of the bound the GPU test uses (the kernel's sums run in yet another order).  If it does not: change the inputs, not the bound.

Output: tests/golden/nav_metrics.npz plus nav_metrics.json (the id strings).    python tests/golden/make_golden_metrics.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

PR = [(1, 1), (1, 5), (2, 2), (7, 6), (63, 5), (64, 64), (65, 64), (130, 65), (40, 200)]
COLS = ['nav_error', 'oracle_error', 'trajectory_steps', 'trajectory_lengths', 'gt_lengths', 'success', 'oracle_success', 'spl', 'DTW', 'nDTW',
        'SDTW', 'CLS']
SUMMED = (3, 4, 7, 9, 10, 11)
MARGIN = 3.0


def import_envs():
    ref_shim._install_common()
    for name in ('MatterSim', 'jsonlines', 'h5py', 'spacy', 'nltk', 'line_profiler', 'sklearnex'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['sklearnex'].patch_sklearn = lambda *a, **k: None
    p = ref_shim.REF_ROOT + '/map_nav_src'
    if p not in sys.path:
        sys.path.insert(0, p)
    import r2r.env as r2r_env
    import reverie.env as reverie_env
    return r2r_env, reverie_env


def make_scans():
    from vln_goat_amd import rollout
    vp = ['grid_vp%03d' % i for i in range(12)]                  # 3 x 4 grid, spacing 3.0: every edge is exactly 3.0 long
    pos = [[3.0 * (i % 4), 3.0 * (i // 4), 0.0] for i in range(12)]
    edges = [(vp[i], vp[i + 1]) for i in range(12) if i % 4 != 3] + [(vp[i], vp[i + 4]) for i in range(8)]
    return [rollout.ScanGraph('grid', vp, pos, edges), rollout.ScanGraph.synthetic('scanM', n=33, seed=21, degree=3),
            rollout.ScanGraph.synthetic('scanL', n=60, seed=22, degree=3)]


def reference_tables(scan):
    """dict of dicts as r2r/env.py:183-189 holds it, and the same values as an [n, n] array in the order of scan.vpids."""
    import networkx as nx
    G = nx.Graph()
    for i, a in enumerate(scan.vpids):
        for j in scan.adj[i]:
            pa, pb = scan.pos[i], scan.pos[j]
            w = ((float(pa[0]) - float(pb[0])) ** 2 + (float(pa[1]) - float(pb[1])) ** 2 + (float(pa[2]) - float(pb[2])) ** 2) ** 0.5       # utils/data.py:79-83
            G.add_edge(a, scan.vpids[j], weight=w)
    d = dict(nx.all_pairs_dijkstra_path_length(G))
    return d, np.array([[d[a][b] for b in scan.vpids] for a in scan.vpids], np.float64)


def walk(scan, rs, start, n, back=0.0):
    """random walk of n nodes over the scan's edges; with probability `back` a step returns to the previous node (a backtrack)."""
    out = [start]
    while len(out) < n:
        nb = scan.adj[out[-1]]
        if len(out) >= 2 and rs.uniform() < back:
            out.append(out[-2])
        else:
            out.append(int(nb[rs.randint(len(nb))]))
    return out


def hops(path, rs):
    """a flat node list as the agent's trajectory: [[start], hop, hop, ...], hops of 1-3 nodes"""
    out, k = [[path[0]]], 1
    while k < len(path):
        n = int(rs.randint(1, 4))
        out.append(path[k:k + n])
        k += n
    return out


def reversed_restatement(D, path, gt, success):
    """columns SUMMED with every sum taken in reverse order (plain Python accumulation from the last term)"""
    def rsum(xs):
        s = 0.0
        for x in reversed(list(xs)):
            s += x
        return s
    tl = rsum(D[a][b] for a, b in zip(path[:-1], path[1:]))
    gl = rsum(D[a][b] for a, b in zip(gt[:-1], gt[1:]))
    spl = success * gl / max(tl, gl, 0.01)
    dtw = np.inf * np.ones((len(path) + 1, len(gt) + 1))
    dtw[0][0] = 0
    for i in range(1, len(path) + 1):
        for j in range(1, len(gt) + 1):
            dtw[i][j] = D[path[i - 1]][gt[j - 1]] + min(dtw[i - 1][j], dtw[i][j - 1], dtw[i - 1][j - 1])
    ndtw = np.exp(-dtw[-1][-1] / (MARGIN * len(gt)))
    with np.errstate(invalid='ignore'):
        cov = rsum(np.exp(-min(D[u][v] for v in path) / MARGIN) for u in gt) / len(gt)
        exp_ = cov * gl
        cls = cov * (np.float64(exp_) / (exp_ + np.abs(exp_ - tl)))
    return {3: tl, 4: gl, 7: spl, 9: ndtw, 10: success * ndtw, 11: cls}


def main():
    r2r_env, reverie_env = import_envs()
    scans = make_scans()
    rs = np.random.RandomState(31)
    tables, out = {}, {}
    ids = {'scans': [], 'cols': COLS, 'margin': MARGIN}
    for k, sc in enumerate(scans):
        tables[sc.name], out['dist_%d' % k] = reference_tables(sc)
        out['pos_%d' % k] = sc.pos
        out['edges_%d' % k] = np.array([(i, j) for i in range(len(sc.vpids)) for j in sc.adj[i] if i < j], np.int64)
        ids['scans'].append({'name': sc.name, 'vpids': sc.vpids})

    # ---- R2R items: every (P, R) twice, on rotating scans (neighbouring items sit on different scans) ----
    items = []
    for rep in range(2):
        for q, (P, R) in enumerate(PR):
            k = (q + rep) % 3
            sc = scans[k]
            start = int(rs.randint(len(sc.vpids)))
            gt = walk(sc, rs, start, R)
            items.append((k, walk(sc, rs, start, P, back=0.3), gt))
    # the strict margin: on the grid, paths that end one edge (exactly 3.0), two edges and zero edges from the goal
    g = scans[0]
    ix = g.index
    for end in ('grid_vp002', 'grid_vp003', 'grid_vp007', 'grid_vp011'):
        items.append((0, [ix['grid_vp000'], ix['grid_vp001'], ix['grid_vp002']] + ([ix[end]] if end != 'grid_vp002' else []),
                      [ix['grid_vp000'], ix['grid_vp001'], ix['grid_vp002'], ix['grid_vp003']]))
    me = types.SimpleNamespace(shortest_distances=tables, gt_trajs={})
    me._get_nearest = types.MethodType(r2r_env.R2RNavBatch._get_nearest, me)
    me._eval_item = types.MethodType(r2r_env.R2RNavBatch._eval_item, me)
    preds = []
    for n, (k, path, gt) in enumerate(items):
        sc = scans[k]
        iid = 'item%03d_0' % n
        me.gt_trajs[iid] = (sc.name, [sc.vpids[v] for v in gt])
        preds.append({'instr_id': iid, 'trajectory': hops([sc.vpids[v] for v in path], rs)})
    with np.errstate(invalid='ignore'):
        avg, metrics = r2r_env.R2RNavBatch.eval_metrics(me, preds)
    N = len(items)
    ref = np.zeros((N, len(COLS)), np.float64)
    worst = 0.0
    for n, (k, path, gt) in enumerate(items):
        sc = scans[k]
        D = tables[sc.name]
        for c, name in enumerate(COLS):
            if name != 'gt_lengths':
                ref[n, c] = metrics[name][n]
        # (the reference keeps gt_lengths in a local: M/r2r/env.py:479, the same expression)
        gtv = me.gt_trajs[preds[n]['instr_id']][1]
        ref[n, 4] = np.sum([D[a][b] for a, b in zip(gtv[:-1], gtv[1:])])
        rev = reversed_restatement(D, [sc.vpids[v] for v in path], gtv, ref[n, 5])
        for c in SUMMED:
            if not (np.isnan(ref[n, c]) and np.isnan(rev[c])):
                worst = max(worst, abs(rev[c] - ref[n, c]) / max(1.0, abs(ref[n, c])))
    assert worst < 1e-13, 'reversed summation order deviates by %.3e: change the inputs' % worst
    assert (ref[:, 0] == 3.0).any() and (ref[:, 0] < 3.0).any() and (ref[:, 0] > 3.0).any()
    assert np.isnan(ref[:, 11]).sum() >= 1                  # the one-node reference path
    ids['reversed_order_max_rel_dev'] = worst
    out['item_scan'] = np.array([k for k, _, _ in items], np.int32)
    out['pred'] = np.concatenate([np.asarray(p, np.int32) for _, p, _ in items])
    out['pred_start'] = np.concatenate([[0], np.cumsum([len(p) for _, p, _ in items])]).astype(np.int32)
    out['ref'] = np.concatenate([np.asarray(r, np.int32) for _, _, r in items])
    out['ref_start'] = np.concatenate([[0], np.cumsum([len(r) for _, _, r in items])]).astype(np.int32)
    out['ref_cols'] = ref
    out['action_steps'] = np.asarray(metrics['action_steps'], np.float64)
    ids['avg_keys'] = list(avg.keys())
    out['avg_vals'] = np.array([avg[k] for k in avg], np.float64)
    ids['preds'] = preds
    ids['gt_trajs'] = {k: [v[0], v[1]] for k, v in me.gt_trajs.items()}

    # ---- REVERIE items: goal sets of 1 and 4 viewpoints, the last node inside / outside ----
    rme = types.SimpleNamespace(shortest_distances=tables, gt_trajs={}, obj2vps={})
    rme._eval_item = types.MethodType(reverie_env.ReverieObjectNavBatch._eval_item, rme)
    rpreds, goal, goal_start, ritems = [], [], [0], []
    pick = [n for n, (k, p, r) in enumerate(items) if len(p) >= 2][:8]
    for m, n in enumerate(pick):
        k, path, gt = items[n]
        sc = scans[k]
        size, inside = (1, 4)[m % 2], (m // 2) % 2 == 0
        others = [v for v in range(len(sc.vpids)) if v != path[-1]]
        if m >= 4:                        # the last node outside the set but an earlier node inside: oracle success without success
            others = [path[0]] + [v for v in others if v not in path]
        gset = ([path[-1]] + others[:size - 1]) if inside else others[:size]
        objid = 100 + m
        iid = 'rv%03d_0' % m
        rme.gt_trajs[iid] = (sc.name, [sc.vpids[v] for v in gt], objid)
        rme.obj2vps['%s_%s' % (sc.name, objid)] = [sc.vpids[v] for v in gset]
        rpreds.append({'instr_id': iid, 'trajectory': preds[n]['trajectory'], 'pred_objid': (objid if m % 3 else (None if m == 0 else str(objid + 1)))})
        goal += gset
        goal_start.append(len(goal))
        ritems.append(n)
    ravg, rmetrics = reverie_env.ReverieObjectNavBatch.eval_metrics(rme, rpreds)
    out['rv_items'] = np.asarray(ritems, np.int32)
    out['rv_goal'], out['rv_goal_start'] = np.asarray(goal, np.int32), np.asarray(goal_start, np.int32)
    for name in ('action_steps', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success', 'spl', 'rgs', 'rgspl'):
        out['rv_' + name] = np.asarray(rmetrics[name], np.float64)
    assert set(out['rv_success']) == {0.0, 1.0} and (out['rv_oracle_success'] > out['rv_success']).any()
    ids['rv_avg_keys'] = list(ravg.keys())
    out['rv_avg_vals'] = np.array([ravg[k] for k in ravg], np.float64)
    ids['rv_preds'] = rpreds
    ids['rv_gt_trajs'] = {k: [v[0], v[1], v[2]] for k, v in rme.gt_trajs.items()}
    ids['rv_obj2vps'] = rme.obj2vps
    np.savez_compressed(os.path.join(HERE, 'nav_metrics.npz'), **out)
    with open(os.path.join(HERE, 'nav_metrics.json'), 'w') as f:
        json.dump(ids, f)
    print('wrote nav_metrics.npz: %d R2R items, %d REVERIE items; reversed-order deviation %.3e; nav_error == 3.0 in %d items; avg %s'
          % (N, len(ritems), worst, int((ref[:, 0] == 3.0).sum()), {k: round(float(v), 4) for k, v in avg.items()}))


if __name__ == '__main__':
    main()
