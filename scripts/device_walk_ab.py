"""A/B of the policy-driven walks with the host planner and with the device navigator (navdev.DeviceNavigator), same process, same graphs.
-> profiles/device_walk_ab.txt

Config-4 R2R model (6 language / 3 cross-modal / 2 panorama layers, BACL + FACL on, vocabulary 50265), bf16, B = 12, T = 15, panorama
width 40, map bucket 64, two synthetic scans of 60 viewpoints, NEW episodes in every iteration.  Timed, each with navigator=None and
navigator=<DeviceNavigator>, the two forms alternating:

  * iteration    SinglePassSampledEpisode.run: the sampled half of a DAgger iteration (instruction graph, 15 step graphs, the walk's
                 decisions, the captured backward graph), device-synchronised.  The teacher graph that follows it in training is the same
                 in both forms and is not part of the A/B.
  * walk         the same call with the backward graph left out (its replay stubbed): the walk alone.
  * argmax       ArgmaxEpisode.run: the validation walk.  The host form stops replaying once every episode has ended; the device form
                 does the same with check_every=1 (one int read per step), and replays all 15 steps without it ('argmax-all').

Host clock around one call that ends synchronised; 2 warm-up calls, then 5 timed per form; median and min-max.  Also: seconds of host
table / packing work per walk (`host_s`) and what the navigator launches per step.

    python scripts/device_walk_ab.py [--out profiles/device_walk_ab.txt]

The measurement runs in a child process under its own `timeout -k 10`; after a step that fails nothing further is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, W, G, L = 12, 15, 40, 64, 80
WARMUP, REPS = 2, 5


def measure():
    import numpy as np
    import torch
    import vln_goat_amd
    from vln_goat_amd import features, hipops, layers, nav_model, rollout, synth
    if not torch.cuda.is_available():
        raise SystemExit('device_walk_ab needs a GPU (no timing without one)')
    a = SimpleNamespace(num_l_layers=6, num_x_layers=3, num_pano_layers=2, dropout=0.1, feat_dropout=0.5, vocab_size=50265, do_back_img=True,
                        do_back_txt=True, do_front_img=True, do_front_his=True, do_front_txt=True, do_back_txt_type='type_2',
                        do_back_img_type='type_1', do_add_method='door', mode='train')
    torch.manual_seed(0)
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(a)).cuda().train()
    vln_goat_amd.set_compute_dtype(torch.bfloat16)
    hipops.manual_seed(4321)
    hipops.RngState.dev = torch.zeros(1, dtype=torch.int64, device='cuda')
    scans = [rollout.ScanGraph.synthetic('scanA', n=60, seed=1, degree=3), rollout.ScanGraph.synthetic('scanB', n=60, seed=2, degree=3)]
    rs = np.random.RandomState(0)
    store = features.FeatureStore.from_arrays({'%s_%s' % (sc.name, vp): rs.standard_normal((36, 768)).astype(np.float32)
                                               for sc in scans for vp in sc.vpids}, dtype=torch.bfloat16).to('cuda')
    _, _, _, dicts = synth.make_rollout_case()
    extras = synth.rollout_extras(dicts, B, 'cuda')
    sim = rollout.GraphSim(store)
    call = lambda mode, batch: model(mode, batch)

    def episodes(it):
        r = np.random.RandomState(1000 + it)
        eps = []
        for k, sc in enumerate(scans):
            eps += synth.rollout_episodes(sc, r, B=B // 2, max_steps=7, starts=[int(x) for x in r.randint(0, len(sc.vpids), B // 2)])
        for i, e in enumerate(eps):
            e['instr_id'] = 'it%d_ep%d' % (it, i)
        return eps
    te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=L, pano_width=W, gmap_width=lambda t: G)
    bufs = rollout.EpisodeBuffers(te.plan(episodes(0)))
    tables = rollout.ScanTables(scans, store)
    walk = rollout.ArgmaxEpisode(te, call, bufs, extras)
    nav_a = rollout.DeviceNavigator(te, tables, bufs, 'argmax')
    params = list(model.parameters())
    sp = rollout.SinglePassSampledEpisode(te, call, bufs, extras)
    nav_s = rollout.DeviceNavigator(te, tables, bufs, 'sample')
    bwd = sp.g_bwd
    noop = SimpleNamespace(replay=lambda: None)
    rng = np.random.RandomState(17)

    def single(nav, with_bwd):
        def fn(eps):
            sp.g_bwd = bwd if with_bwd else noop
            sp.run(eps, rng, navigator=nav)
            return sp.host_s, sp.steps
        return fn

    def argmax(nav, check=None):
        def fn(eps):
            walk.run(eps, navigator=nav, check_every=check)
            return walk.host_s, walk.steps
        return fn
    forms = {'iteration/host': single(None, True), 'iteration/device': single(nav_s, True), 'walk/host': single(None, False),
             'walk/device': single(nav_s, False), 'argmax/host': argmax(None), 'argmax/device': argmax(nav_a, 1), 'argmax-all/device': argmax(nav_a)}
    times = {k: [] for k in forms}
    host = {k: [] for k in forms}
    steps = {k: [] for k in forms}
    for it in range(WARMUP + REPS):
        eps = episodes(it + 1)
        for name, fn in forms.items():
            for p in params:
                if p.grad is not None:
                    p.grad.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h, n = fn(eps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= WARMUP:
                times[name].append(dt * 1e3), host[name].append(h * 1e3), steps[name].append(n)
    sp.g_bwd = bwd
    refreshed = [sum(1 for ent in layers._MASK_MEMO.values() if ent[0]() is not None and any(ent[0]() is x for x in nav_s._step_tensors[t])) for t in range(T)]
    print('RESULT ' + json.dumps({'times': times, 'host': host, 'steps': steps, 'kernels_per_step': nav_s.launches_per_step,
                                  'masks_refreshed_per_step': refreshed}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_walk_ab.txt'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return measure()
    r = subprocess.run(['timeout', '-k', '10', '540', sys.executable, os.path.abspath(__file__), '--child'], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    res = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    if r.returncode != 0 or not res:
        print(r.stdout[-4000:])
        raise SystemExit('timing step failed (exit status %d): nothing further is run on the GPU' % r.returncode)
    d = json.loads(res[-1][7:])
    lines = ['policy-driven walks, host planner against device navigator: config-4 R2R model, bf16, B = %d, T = %d, W = %d, map bucket %d,' % (B, T, W, G),
             'new episodes per iteration.  Wall time of one call, device-synchronised; %d warm-up calls, %d timed, forms alternating.' % (WARMUP, REPS), '']
    med = {}
    for name in d['times']:
        t = d['times'][name]
        med[name] = statistics.median(t)
        lines.append('%-18s median %8.2f ms   min %8.2f   max %8.2f   host work %6.2f ms per walk   steps %4.1f   (%s)'
                     % (name, med[name], min(t), max(t), statistics.median(d['host'][name]), statistics.mean(d['steps'][name]), ', '.join('%.2f' % x for x in t)))
    lines.append('')
    slower = []
    for what in ('iteration', 'walk', 'argmax'):
        ratio = med[what + '/device'] / med[what + '/host']
        lines.append('%-10s median(device) / median(host) = %.3f' % (what, ratio))
        if ratio > 1.0:
            slower.append(what)
    lines.append('%-10s median(device, all %d steps, no read) / median(host) = %.3f' % ('argmax', T, med['argmax-all/device'] / med['argmax/host']))
    lines += ['', 'the device navigator launches %d kernels per step (goat_nav_step: one workgroup per episode, one for the compact CSRs) and recomputes %s '
              'memoised masks per step (a few element-wise torch launches each); the host form makes one H2D copy and one synchronising read-back per step.'
              % (d['kernels_per_step'], '%d-%d' % (min(d['masks_refreshed_per_step']), max(d['masks_refreshed_per_step']))),
              'device form not slower than the host form: %s' % ('yes' if not slower else 'NO (%s)' % ', '.join(slower))]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
