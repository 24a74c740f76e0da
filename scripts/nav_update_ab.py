"""Times the fine-tuning update on the config-4 model and its 'nav' gradient arena and writes profiles/nav_update_ab.txt.

    python scripts/nav_update_ab.py [--no-trace] [--out profiles/nav_update_ab.txt]

Three forms of one update (clip 40, AdamW with torch's defaults) over the parameters a navigation episode gives a gradient:
  (a) optim.FusedTorchOptim.step()              goat_grad_sqnorm, goat_optim_step, goat_optim_advance
  (b) the same step replayed from a hipGraph    captured once through hipops.graph
  (c) what a user has without that class        torch.nn.utils.clip_grad_norm_(params, 40.) + torch.optim.AdamW(params).step() +
                                                hipops.refresh_shadows over every parameter (the captured episode graphs read the
                                                cached bf16 copies at fixed addresses: without it they go stale)
The model is config 4 (6 / 3 / 2 layers, vocabulary 50 265, BACL + FACL, bf16 compute); a two-step episode of two samples supplies the usage
set, the cached operand copies and the gradients — the update's cost depends on the parameter count, not on the episode.  Time between
two device events around each call, median (min .. max) of 20 after 5 warm-ups, one form after the other.  Launch counts: two
`rocprofv3 --kernel-trace --stats` child runs per form (4 updates and 1 update) differenced, so that model construction and the episode
drop out.  Every GPU step is a child process under its own `timeout -k 10`; after a step that fails nothing further is started.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 5, 20


def _setup():
    import torch
    import vln_goat_amd
    from vln_goat_amd import dp, hipops, nav_model, optim, synth
    if not torch.cuda.is_available():
        raise SystemExit('nav_update_ab.py measures on the GPU: none found')
    a = SimpleNamespace(num_l_layers=6, num_x_layers=3, num_pano_layers=2, dropout=0.1, feat_dropout=0.5, vocab_size=50265,
                        do_back_img=True, do_back_txt=True, do_front_img=True, do_front_his=True, do_front_txt=True,
                        do_back_txt_type='type_2', do_back_img_type='type_1', do_add_method='door', mode='train')
    torch.manual_seed(0)
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(a)).cuda().eval()
    vln_goat_amd.set_compute_dtype(torch.bfloat16)
    ep = synth.make_nav_episode(B=2, L=40, n_steps=2, seed=21, vocab_size=50265)
    mv = lambda x: x.cuda() if torch.is_tensor(x) else x
    ep = {k: ([{kk: mv(vv) for kk, vv in st.items()} for st in v] if k == 'steps' else mv(v)) for k, v in ep.items()}

    def episode():
        loss, _ = synth.run_nav_episode(lambda m, b: model(m, b), ep, device='cuda')
        loss.backward()
    episode()
    wrapper = dp.GoatDataParallel(model)
    wrapper.record_usage('nav')
    for p in model.parameters():
        p.grad = None
    arena = wrapper.build_arena()
    arena.zero('nav')
    episode()
    torch.cuda.synchronize()
    params = [p for p in model.parameters() if id(p) in arena.views]
    by_id = {id(p): p for p in model.parameters()}
    fused = optim.FusedTorchOptim(model.named_parameters(), arena, algo='adamW', lr=1e-5)
    topt = torch.optim.AdamW(list(model.parameters()), lr=1e-5)

    def form_a():
        fused.step(max_norm=40.0)

    def form_c():
        torch.nn.utils.clip_grad_norm_(params, 40.)
        topt.step()
        for p in params:
            hipops.refresh_shadows(p, by_id)

    info = {'device': torch.cuda.get_device_name(0), 'tensors': len(params), 'elements': int(sum(p.numel() for p in params)),
            'chunks': fused._tb.nchunks, 'copies': int(sum(len(p.__dict__.get('_goat_shadow') or {}) for p in params))}
    return torch, hipops, fused, form_a, form_c, info


def _time(torch, fn):
    out = []
    for i in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            out.append(e0.elapsed_time(e1))
    return out


def measure():
    torch, hipops, fused, form_a, form_c, info = _setup()
    times = {'a': _time(torch, form_a)}
    info['refreshed_after_a'] = fused.last_refreshed
    g = torch.cuda.CUDAGraph()
    with hipops.graph(g):
        form_a()
    times['b'] = _time(torch, g.replay)
    times['c'] = _time(torch, form_c)
    info['steps_done'] = fused.steps_done()
    print('RESULT ' + json.dumps({'times': times, 'info': info}))


def count(form, n):
    torch, hipops, fused, form_a, form_c, info = _setup()
    for _ in range(n):
        (form_a if form == 'a' else form_c)()
    torch.cuda.synchronize()


def _run(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nav_update_ab.txt'))
    ap.add_argument('--child', choices=['measure', 'count-a', 'count-c'])
    ap.add_argument('--updates', type=int, default=4, help='(count children) updates per run')
    ap.add_argument('--no-trace', action='store_true', help='skip the four rocprofv3 runs (launch counts)')
    a = ap.parse_args()
    if a.child == 'measure':
        return measure()
    if a.child:
        return count(a.child.split('-')[1], a.updates)

    me = [sys.executable, os.path.abspath(__file__)]
    rc, out = _run(me + ['--child', 'measure'], 420)
    res = [ln for ln in out.splitlines() if ln.startswith('RESULT ')]
    if rc != 0 or not res:
        print(out[-4000:])
        raise SystemExit('timing step failed (exit status %d): nothing further is run on the GPU' % rc)
    r = json.loads(res[-1][7:])
    times, info = r['times'], r['info']
    print('timing step done', flush=True)
    lines = ['fine-tuning update A/B (scripts/nav_update_ab.py): clip_grad_norm_ 40 + AdamW (torch defaults, lr 1e-5) on the config-4 model, bf16 compute',
             'device: %s   %d tensors, %d elements in %d chunks, %d cached operand copies; %d of them rebuilt by torch ops after the fused kernel'
             % (info['device'], info['tensors'], info['elements'], info['chunks'], info['copies'], info['refreshed_after_a']),
             'time between two device events around one update, median of %d after %d warm-ups (min .. max); one run on one box' % (REPS, WARMUP), '']
    stat = {}
    for k, label in (('a', '(a) FusedTorchOptim.step(), eager'), ('b', '(b) the same step replayed from a hipGraph'),
                     ('c', '(c) clip_grad_norm_ + torch.optim.AdamW.step() + refresh_shadows')):
        t = times[k]
        stat[k] = statistics.median(t)
        lines.append('%-70s %9.3f ms (%.3f .. %.3f)' % (label, stat[k], min(t), max(t)))
    lines += ['', 'median (c) / median (a) = %.2f;  median (c) / median (b) = %.2f;  bytes moved by (a) at 32 B per element: %.1f MB'
              % (stat['c'] / stat['a'], stat['c'] / stat['b'], info['elements'] * 32 / 1e6)]
    trace_failed = False
    if not a.no_trace:
        lines.append('')
        for form in ('a', 'c'):
            rows = {}
            for n in (a.updates, 1):
                with tempfile.TemporaryDirectory() as d:
                    rc, out = _run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--'] + me
                                   + ['--child', 'count-' + form, '--updates', str(n)], 420)
                    f = glob.glob(d + '/**/*kernel_stats.csv', recursive=True)
                    if rc != 0 or not f:
                        lines.append('launch count (%s, %d updates): rocprofv3 run failed (exit status %d)' % (form, n, rc))
                        print(out[-3000:])
                        trace_failed = True
                        break
                    rows[n] = {row['Name']: int(row['Calls']) for row in csv.DictReader(open(f[0]))}
                    print('kernel trace (%s, %d updates) done' % (form, n), flush=True)
            if trace_failed:
                break                                       # nothing further on the GPU after a failed step
            full, base = rows[a.updates], rows[1]
            steps = a.updates - 1
            per = {k: (v - base.get(k, 0)) / steps for k, v in full.items()}
            top = sorted(per.items(), key=lambda kv: -kv[1])[:4]
            lines.append('launches per update (%s): %.1f  = (%d dispatches in a run of %d updates - %d in a run of 1) / %d; most frequent: %s'
                         % (form, (sum(full.values()) - sum(base.values())) / steps, sum(full.values()), a.updates, sum(base.values()), steps,
                            '; '.join('%s x%.1f' % (k[:56], v) for k, v in top)))
        if not trace_failed:
            lines.append('(b) replays the three launches of (a) as one graph launch')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write(text)
    if trace_failed:
        raise SystemExit(3)


if __name__ == '__main__':
    main()
