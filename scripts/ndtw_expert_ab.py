"""What the nDTW expert costs per step, on the host and on the device.  -> profiles/ndtw_expert.txt

A walk shaped like the config-4 leg: B = 12, T = 15, panorama width 40, map bucket 64, ground-truth bucket max_ref = 32, two synthetic
scans of 60 viewpoints, RxR-style ground-truth paths (synth.rxr_episodes), the actions of a seeded random policy over the selectable
nodes (what a sampled walk does to the navigator), NEW episodes in every repetition.  No model: only the navigator is timed.

  * host      nav_inputs.teacher_action(expert_policy='ndtw') of every step of the host planner's walk, host clock, per step.
  * device    hipEvents around the loop of launches `for t in 0..T: DeviceNavigator.step(t)` (forced mode, the same actions), once with a
              'spl' navigator — goat_nav_step alone, what the tree launched before — and once with an 'ndtw' navigator (goat_nav_step +
              goat_nav_ndtw), the two alternating on the same episodes.  Per step = loop time / T.

3 warm-up repetitions, then 20 timed; median and min-max.

    python scripts/ndtw_expert_ab.py [--out profiles/ndtw_expert.txt]

The measurement runs in a child process under its own `timeout -k 10`; after a step that fails nothing further is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, W, G, MAX_REF = 12, 15, 40, 64, 32
WARMUP, REPS = 3, 20


def measure():
    import numpy as np
    import torch
    from vln_goat_amd import nav_inputs, rollout, synth
    if not torch.cuda.is_available():
        raise SystemExit('ndtw_expert_ab needs a GPU (no timing without one)')
    scans = [rollout.ScanGraph.synthetic('scanA', n=60, seed=1, degree=3), rollout.ScanGraph.synthetic('scanB', n=60, seed=2, degree=3)]
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    sim = rollout.GraphSim(rollout._RowIndex(keys))
    te = {pol: rollout.TeacherEpisode(sim, None, n_steps=T, text_len=80, pano_width=W, gmap_width=lambda t: G, expert_policy=pol)
          for pol in ('spl', 'ndtw')}

    def episodes(it):
        r = np.random.RandomState(1000 + it)
        eps = []
        for sc in scans:
            eps += synth.rxr_episodes(sc, r, B=B // 2, max_ref=MAX_REF, n_way=4, starts=[int(x) for x in r.randint(0, len(sc.vpids), B // 2)])
        for i, e in enumerate(eps):
            e['instr_id'] = 'it%d_ep%d' % (it, i)
        return eps

    def host_walk(eps, it):
        """the host planner under the random policy -> (actions, seconds in teacher_action('ndtw'), labelled states, steps with a live episode)"""
        rs = np.random.RandomState(2000 + it)
        p = rollout.EpisodePlanner(te['spl'], eps, imitation=False)
        acts, secs, labelled, live = [], 0.0, 0, 0
        for t in range(T):
            part = p.build_step()
            live += not p.ended.all()
            t0 = time.perf_counter()
            lab = nav_inputs.teacher_action(p.obs, p._gin['gmap_vpids'], p.ended, p._gin['gmap_visited_masks'].numpy(), False, t, te['spl'].ignoreid,
                                            expert_policy='ndtw', traj=p.traj)
            secs += time.perf_counter() - t0
            labelled += int((lab > 0).sum())
            sel = (part['s%d_gmap_masks' % t] & ~part['s%d_gmap_visited_masks' % t]).numpy()
            a = np.zeros(B, np.int64)
            for b in range(B):
                slots = np.nonzero(sel[b, 2:])[0] + 2
                a[b] = 0 if (p.ended[b] or not len(slots)) else int(slots[rs.randint(len(slots))])
            p.advance(a)
            acts.append(a)
        return acts, secs, labelled, live

    bufs = rollout.EpisodeBuffers(te['spl'].plan(episodes(0)))
    tables = rollout.ScanTables(scans, sim.features)
    nav = {'spl': rollout.DeviceNavigator(te['spl'], tables, bufs, 'forced'),
           'ndtw': rollout.DeviceNavigator(te['ndtw'], tables, bufs, 'forced', max_ref=MAX_REF)}
    ms = {'spl': [], 'ndtw': []}
    host_ms, labelled, live = [], [], []
    for it in range(WARMUP + REPS):
        eps = episodes(it + 1)
        acts, secs, n_lab, n_live = host_walk(eps, it)
        for pol in (('spl', 'ndtw') if it % 2 == 0 else ('ndtw', 'spl')):
            n = nav[pol]
            n.begin(eps, actions=acts)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(T + 1):
                n.step(t)
            e1.record()
            n.finish()                      # (synchronises; raises on a status word)
            if it >= WARMUP:
                ms[pol].append(e0.elapsed_time(e1))
        if it >= WARMUP:
            host_ms.append(secs * 1e3)
            labelled.append(n_lab)
            live.append(n_live)
    print('RESULT ' + json.dumps({'ms': ms, 'host_ms': host_ms, 'labelled': labelled, 'live': live, 'box': '%s (%s)' % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
                                  'launches': {k: v.launches_per_step for k, v in nav.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ndtw_expert.txt'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return measure()
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--child'], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    res = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    if r.returncode != 0 or not res:
        print(r.stdout[-4000:])
        raise SystemExit('timing step failed (exit status %d): nothing further is run on the GPU' % r.returncode)
    d = json.loads(res[-1][7:])
    med = {k: statistics.median(v) for k, v in d['ms'].items()}
    host = statistics.median(d['host_ms'])
    fmt = lambda v: 'median %8.3f ms   min %8.3f   max %8.3f' % (statistics.median(v), min(v), max(v))
    lines = ['nDTW expert per step, host against device: B = %d, T = %d, W = %d, map bucket %d, max_ref = %d, two synthetic scans of 60 viewpoints,' % (B, T, W, G, MAX_REF),
             'RxR-style ground-truth paths, random-policy actions, new episodes per repetition; %d warm-up repetitions, %d timed, the two device' % (WARMUP, REPS),
             'forms alternating.  Box: %s.  Command: python scripts/ndtw_expert_ab.py' % d['box'], '',
             'host    teacher_action(expert_policy=\'ndtw\'), all %d steps of a walk (host clock)      %s' % (T, fmt(d['host_ms'])),
             'device  loop of launches, \'spl\'  navigator (%d launches per step; hipEvents)           %s' % (d['launches']['spl'], fmt(d['ms']['spl'])),
             'device  loop of launches, \'ndtw\' navigator (%d launches per step; hipEvents)           %s' % (d['launches']['ndtw'], fmt(d['ms']['ndtw'])), '',
             'per step (walk / %d):  host teacher_action %.3f ms   device \'spl\' %.4f ms   device \'ndtw\' %.4f ms   added by goat_nav_ndtw %.4f ms'
             % (T, host / T, med['spl'] / T, med['ndtw'] / T, (med['ndtw'] - med['spl']) / T),
             'labelled states per walk (label > 0): median %d; steps with a live episode: median %d of %d' % (
                 statistics.median(d['labelled']), statistics.median(d['live']), T),
             'no model and no step graph here, so no memoised mask exists that a navigator step would refresh: the device loop is the navigator kernels alone.']
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
