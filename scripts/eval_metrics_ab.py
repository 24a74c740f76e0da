"""Times the validation pass in its two forms and writes profiles/eval_metrics_ab.txt.

    python scripts/eval_metrics_ab.py [--dtype bf16] [--items 7047] [--out profiles/eval_metrics_ab.txt]

  walk      the eager rollout.NavRollout.run(feedback='argmax', compute_loss=False) — what the parent commit offers for validation —
            against rollout.ArgmaxEpisode (captured step graphs), config-4 shape: the full-size R2R navigation model (without the confounder
            dictionaries), B = 12, T = 15,
            four synthetic 60-viewpoint scans, model.eval(), new episodes every call, the same episodes for both forms.
  metrics   a Python restatement of the reference's per-item scoring (dict-of-dict tables, the DTW and CLS double loops of
            M/r2r/eval_utils.py) against evaluate.NavEvaluator.eval_metrics (flatten, one upload, goat_nav_metrics, one read-back) over
            2 349 x 3 synthetic items (the size of R2R val_unseen): ground-truth shortest paths, predictions = random walks with backtracks.

Each of the three GPU steps is a child process under its own `timeout -k 10`; the parent stops at the first that fails.  Wall clock
around each call with a device synchronise at both ends, median (min .. max) of 5 after 2 warm-ups.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, L, W = 12, 15, 80, 38
N_WARM, N_TIMED = 2, 5
LIMITS = {'eager_walk': 300, 'captured_walk': 300, 'metrics': 300}


def scans_of():
    from vln_goat_amd import rollout
    return [rollout.ScanGraph.synthetic('scan%d' % k, n=60, seed=40 + k, degree=3) for k in range(4)]


def episodes(scans, rs, k):
    eps = []
    for b in range(B):
        sc = scans[(k + b) % len(scans)]
        dist, _ = sc.shortest()
        s0 = int(rs.randint(len(sc.vpids)))
        far = int(np.argsort(dist[s0])[-1 - int(rs.randint(6))])
        n_tok = int(rs.randint(L // 2, L - 1))
        eps.append({'instr_id': 'k%d_b%d' % (k, b), 'scan': sc, 'path': sc.shortest_path(sc.vpids[s0], sc.vpids[far]),
                    'heading': float(rs.uniform(0, 2 * np.pi)), 'instr_encoding': [0] + rs.randint(3, 50000, n_tok - 2).tolist() + [2]})
    return eps


def timed(fn, n_calls):
    import torch
    out = []
    for i in range(n_calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[N_WARM:]


def walk_child(form, dtype):
    import torch
    import vln_goat_amd
    from vln_goat_amd import features, nav_model, rollout, synth
    vln_goat_amd.set_compute_dtype(torch.bfloat16 if dtype == 'bf16' else torch.float32)
    a = SimpleNamespace(num_l_layers=6, num_x_layers=3, num_pano_layers=2, dropout=0.1, feat_dropout=0.5, vocab_size=50265, mode='train')
    torch.manual_seed(0)
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(a))
    model.load_state_dict(synth.seeded_state_dict(model, seed=11))
    model = model.cuda().eval()
    scans = scans_of()
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    store = features.FeatureStore.synthetic(keys, D=768, seed=3, dtype=torch.bfloat16 if dtype == 'bf16' else torch.float32).to('cuda')
    sim = rollout.GraphSim(store)
    rs = np.random.RandomState(31)
    batches = [episodes(scans, rs, k) for k in range(N_WARM + N_TIMED)]
    steps = []
    if form == 'eager_walk':
        ro = rollout.NavRollout(model, sim, store, max_action_len=T, pano_width=W, gmap_buckets=sorted({rollout.default_gmap_width(t) for t in range(T)}))

        def one(i):
            with torch.no_grad():
                _, traj = ro.run(batches[i], feedback='argmax', compute_loss=False)
            steps.append(ro.steps)
            one.traj = traj
    else:
        te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=L, pano_width=W)
        walk = rollout.ArgmaxEpisode(te, model, rollout.EpisodeBuffers(te.plan(batches[0])))

        def one(i):
            one.traj = walk.run(batches[i])
            steps.append(walk.steps)
    ms = timed(one, N_WARM + N_TIMED)
    print(json.dumps({'form': form, 'ms': ms, 'steps': steps[N_WARM:], 'device': torch.cuda.get_device_name(0),
                      'last_paths': [[h[-1] for h in tr['path']] for tr in one.traj]}))


def python_metrics(tables, gt_trajs, preds, margin=3.0):
    """per-item scores and averages as the reference forms them, on its dict-of-dict tables (a restatement; plain Python loops)"""
    rows = []
    for item in preds:
        scan, gt = gt_trajs[item['instr_id']]
        D = tables[scan]
        path = [vp for hop in item['trajectory'] for vp in hop]
        goal = gt[-1]
        nav_error = D[path[-1]][goal]
        oracle_error = min(D[vp][goal] for vp in path)
        length = np.sum([D[a][b] for a, b in zip(path[:-1], path[1:])])
        gt_length = np.sum([D[a][b] for a, b in zip(gt[:-1], gt[1:])])
        success = float(nav_error < margin)
        spl = success * gt_length / max(length, gt_length, 0.01)
        m = np.inf * np.ones((len(path) + 1, len(gt) + 1))
        m[0][0] = 0
        for i in range(1, len(path) + 1):
            for j in range(1, len(gt) + 1):
                m[i][j] = D[path[i - 1]][gt[j - 1]] + min(m[i - 1][j], m[i][j - 1], m[i - 1][j - 1])
        ndtw = np.exp(-m[len(path)][len(gt)] / (margin * len(gt)))
        coverage = np.mean([np.exp(-np.min([D[u][v] for v in path]) / margin) for u in gt])
        expected = coverage * gt_length
        cls = coverage * expected / (expected + np.abs(expected - length))
        rows.append((len(item['trajectory']) - 1, len(path) - 1, length, nav_error, oracle_error, success, float(oracle_error < margin), spl,
                     ndtw, success * ndtw, cls))
    r = np.asarray(rows, np.float64)
    names = ('action_steps', 'steps', 'lengths', 'nav_error', 'oracle_error', 'sr', 'oracle_sr', 'spl', 'nDTW', 'SDTW', 'CLS')
    return {n: float(r[:, c].mean()) * (100 if c >= 5 else 1) for c, n in enumerate(names)}


def metrics_child(n_items):
    import torch
    from vln_goat_amd import evaluate
    scans = scans_of()
    rs = np.random.RandomState(7)
    tables = {sc.name: {a: {b: float(sc.shortest()[0][i, j]) for j, b in enumerate(sc.vpids)} for i, a in enumerate(sc.vpids)} for sc in scans}
    gt_trajs, preds = {}, []
    for n in range(n_items):
        sc = scans[n % len(scans)]
        dist, _ = sc.shortest()
        s0 = int(rs.randint(len(sc.vpids)))
        gt = sc.shortest_path(sc.vpids[s0], sc.vpids[int(np.argsort(dist[s0])[-1 - int(rs.randint(6))])])
        path, hops = [s0], [[sc.vpids[s0]]]
        for _ in range(int(rs.randint(1, T))):                      # up to T - 1 actions of 1-3 viewpoints, some of them backtracks
            hop = []
            for _ in range(int(rs.randint(1, 4))):
                nb = sc.adj[path[-1]]
                path.append(path[-2] if (len(path) > 1 and rs.uniform() < 0.2) else int(nb[rs.randint(len(nb))]))
                hop.append(sc.vpids[path[-1]])
            hops.append(hop)
        iid = 'item%d' % n
        gt_trajs[iid] = (sc.name, gt)
        preds.append({'instr_id': iid, 'trajectory': hops})
    ev = evaluate.NavEvaluator(scans, gt_trajs)
    res = {}

    def dev(i):
        res['device'] = ev.eval_metrics(preds)[0]

    def host(i):
        res['python'] = python_metrics(tables, gt_trajs, preds)
    ms_dev, ms_py = timed(dev, N_WARM + N_TIMED), timed(host, N_WARM + N_TIMED)
    diff = max(abs(res['device'][k] - res['python'][k]) for k in res['python'])
    print(json.dumps({'form': 'metrics', 'device_ms': ms_dev, 'python_ms': ms_py, 'items': n_items, 'max_avg_diff': diff,
                      'avg': {k: float(v) for k, v in res['device'].items()}, 'device': torch.cuda.get_device_name(0),
                      'mean_P': float(np.mean([sum(len(h) for h in p['trajectory']) for p in preds])),
                      'mean_R': float(np.mean([len(v[1]) for v in gt_trajs.values()]))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', choices=('bf16', 'f32'), default='bf16')
    ap.add_argument('--items', type=int, default=2349 * 3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_metrics_ab.txt'))
    ap.add_argument('--child', choices=tuple(LIMITS))
    args = ap.parse_args()
    if args.child in ('eager_walk', 'captured_walk'):
        return walk_child(args.child, args.dtype)
    if args.child == 'metrics':
        return metrics_child(args.items)
    got = {}
    for name in LIMITS:           # every GPU step a fresh child under its own time limit; nothing more is started after one that fails
        cmd = ['timeout', '-k', '10', str(LIMITS[name]), sys.executable, os.path.abspath(__file__), '--child', name, '--dtype', args.dtype,
               '--items', str(args.items)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit('%s ended with status %d: nothing further is run' % (name, r.returncode))
        got[name] = json.loads(r.stdout.strip().splitlines()[-1])
    fmt = lambda t: '%9.2f ms (%.2f .. %.2f)' % (statistics.median(t), min(t), max(t))
    e, c, m = got['eager_walk'], got['captured_walk'], got['metrics']
    n_batches = -(-args.items // B)
    lines = ['validation pass: eager argmax walk + Python metrics against ArgmaxEpisode + NavEvaluator (scripts/eval_metrics_ab.py)',
             'device: %s   compute dtype %s   one run on one box' % (m['device'], args.dtype),
             'wall clock per call, synchronised, median of %d after %d warm-ups (min .. max); every GPU step in a process of its own' % (N_TIMED, N_WARM),
             '',
             'walk: full-size R2R navigation model (6 / 3 / 2 layers, no confounder dictionaries) in eval mode, B = %d, T = %d, panorama width %d, four 60-viewpoint scans, new episodes per call' % (B, T, W),
             '  %-66s %s   steps taken %s' % ('NavRollout.run(feedback=argmax), eager (map buckets of 16)', fmt(e['ms']), e['steps']),
             '  %-66s %s   steps taken %s' % ('ArgmaxEpisode.run, %d captured step graphs (map width 16 (t + 1))' % T, fmt(c['ms']), c['steps']),
             '  the two forms end the last batch on the same viewpoints: %s' % (e['last_paths'] == c['last_paths']),
             '',
             'metrics: %d items, predicted paths of %.1f and ground-truth paths of %.1f viewpoints on average' % (m['items'], m['mean_P'], m['mean_R']),
             '  %-66s %s' % ('Python restatement of the reference (dict tables, DTW / CLS loops)', fmt(m['python_ms'])),
             '  %-66s %s' % ('NavEvaluator.eval_metrics (flatten, upload, goat_nav_metrics, read-back)', fmt(m['device_ms'])),
             '  largest |device - Python| over the eleven averages: %.3e' % m['max_avg_diff'],
             '',
             'a validation pass over %d items = %d batches of %d:' % (args.items, n_batches, B),
             '  eager walk + Python metrics      %9.1f s' % ((n_batches * statistics.median(e['ms']) + statistics.median(m['python_ms'])) / 1e3),
             '  captured walk + NavEvaluator     %9.1f s' % ((n_batches * statistics.median(c['ms']) + statistics.median(m['device_ms'])) / 1e3)]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
