"""A/B of the REVERIE walks with the host planner and with the device navigator (navdev.DeviceNavigator(objects=)), same process, same
graphs, same objects.  -> profiles/reverie_walk_ab.txt

The shapes of the bench's REVERIE navigator leg: config-4 model with the object-grounding head (6 language / 3 cross-modal / 2 panorama
layers, BACL + FACL on, vocabulary 50265), bf16, B = 12, T = 15, panorama width 38 + 20 objects, map bucket 64, four synthetic scans of
60 viewpoints with up to 20 objects per viewpoint, NEW episodes in every iteration (each with its own `obj_id`; GraphSim(obj_fallback=
False)).  Timed, each with navigator=None and navigator=<DeviceNavigator>, the two forms alternating:

  * walk         SinglePassSampledEpisode.run with the backward graph left out (its replay stubbed): the sampled walk alone.
  * argmax       ArgmaxEpisode.run: the validation walk.  The host form stops replaying once every episode has ended; the device form
                 does the same with check_every=1 (one int read per step), and replays all 15 steps without it ('argmax-all').

Host clock around one call that ends synchronised; 2 warm-up calls, then 5 timed per form; median and min-max, and the seconds of host
table / packing work per walk (`host_s`).

    python scripts/reverie_walk_ab.py [--out profiles/reverie_walk_ab.txt]

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
B, T, W, O, G, L = 12, 15, 38, 20, 64, 80
WARMUP, REPS = 2, 5


def measure():
    import numpy as np
    import torch
    import vln_goat_amd
    from vln_goat_amd import features, hipops, nav_model, rollout, synth
    if not torch.cuda.is_available():
        raise SystemExit('reverie_walk_ab needs a GPU (no timing without one)')
    a = SimpleNamespace(num_l_layers=6, num_x_layers=3, num_pano_layers=2, dropout=0.1, feat_dropout=0.5, vocab_size=50265, do_back_img=True,
                        do_back_txt=True, do_front_img=True, do_front_his=True, do_front_txt=True, do_back_txt_type='type_2',
                        do_back_img_type='type_1', do_add_method='door', mode='train', dataset='reverie', obj_feat_size=768)
    torch.manual_seed(0)
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(a)).cuda().train()
    vln_goat_amd.set_compute_dtype(torch.bfloat16)
    hipops.manual_seed(4321)
    hipops.RngState.dev = torch.zeros(1, dtype=torch.int64, device='cuda')
    scans = [rollout.ScanGraph.synthetic('rscan%d' % k, n=60, seed=70 + k, degree=3) for k in range(4)]
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    store = features.FeatureStore.synthetic(keys, D=768, seed=5, dtype=torch.bfloat16).to('cuda')
    objects = rollout.ObjectStore.synthetic(scans, D=768, max_objects=O, seed=9, dtype=torch.bfloat16, p_empty=0.2).to('cuda')
    _, _, _, dicts = synth.make_rollout_case()
    extras = synth.rollout_extras(dicts, B, 'cuda')
    sim = rollout.GraphSim(store, objects=objects, obj_fallback=False)
    call = lambda mode, batch: model(mode, batch)

    def episodes(it):
        r = np.random.RandomState(1000 + it)
        eps = []
        for k, sc in enumerate(scans):
            eps += synth.reverie_episodes(sc, objects, r, B=B // len(scans), max_steps=7,
                                          starts=[int(x) for x in r.randint(0, len(sc.vpids), B // len(scans))])
        for i, e in enumerate(eps):
            e['instr_id'] = 'it%d_ep%d' % (it, i)
        return eps
    te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=L, pano_width=W, gmap_width=lambda t: G, obj_width=O)
    bufs = rollout.EpisodeBuffers(te.plan(episodes(0)))
    tables = rollout.ScanTables(scans, store)
    otab = rollout.ObjectTables(objects, tables)
    walk = rollout.ArgmaxEpisode(te, call, bufs, extras)
    nav_a = rollout.DeviceNavigator(te, tables, bufs, 'argmax', objects=otab)
    sp = rollout.SinglePassSampledEpisode(te, call, bufs, extras)
    nav_s = rollout.DeviceNavigator(te, tables, bufs, 'sample', objects=otab)
    bwd = sp.g_bwd
    sp.g_bwd = SimpleNamespace(replay=lambda: None)
    rng = np.random.RandomState(17)

    def single(nav):
        def fn(eps):
            sp.run(eps, rng, navigator=nav)
            return sp.host_s, sp.steps
        return fn

    def argmax(nav, check=None):
        def fn(eps):
            walk.run(eps, navigator=nav, check_every=check)
            return walk.host_s, walk.steps
        return fn
    forms = {'walk/host': single(None), 'walk/device': single(nav_s), 'argmax/host': argmax(None), 'argmax/device': argmax(nav_a, 1),
             'argmax-all/device': argmax(nav_a)}
    times = {k: [] for k in forms}
    host = {k: [] for k in forms}
    steps = {k: [] for k in forms}
    for it in range(WARMUP + REPS):
        eps = episodes(it + 1)
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h, n = fn(eps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= WARMUP:
                times[name].append(dt * 1e3), host[name].append(h * 1e3), steps[name].append(n)
    sp.g_bwd = bwd
    print('RESULT ' + json.dumps({'times': times, 'host': host, 'steps': steps, 'kernels_per_step': nav_s.launches_per_step}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reverie_walk_ab.txt'))
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
    lines = ['REVERIE walks, host planner against device navigator: config-4 model with the object head, bf16, B = %d, T = %d, W = %d + %d objects,'
             % (B, T, W, O), 'map bucket %d, new episodes per iteration.  Wall time of one call, device-synchronised; %d warm-up calls, %d timed, '
             'forms alternating.' % (G, WARMUP, REPS), '']
    med = {}
    for name in d['times']:
        t = d['times'][name]
        med[name] = statistics.median(t)
        lines.append('%-18s median %8.2f ms   min %8.2f   max %8.2f   host work %6.2f ms per walk   steps %4.1f   (%s)'
                     % (name, med[name], min(t), max(t), statistics.median(d['host'][name]), statistics.mean(d['steps'][name]), ', '.join('%.2f' % x for x in t)))
    lines.append('')
    for what in ('walk', 'argmax'):
        lines.append('%-10s median(device) / median(host) = %.3f' % (what, med[what + '/device'] / med[what + '/host']))
    lines.append('%-10s median(device, all %d steps, no read) / median(host) = %.3f' % ('argmax', T, med['argmax-all/device'] / med['argmax/host']))
    lines += ['', 'the device navigator launches %d kernels per step (goat_nav_obj_step: one workgroup per episode, one for the compact CSRs and the '
              'object concat index); the host form makes one H2D copy and one synchronising read-back per step.' % d['kernels_per_step']]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
