"""A/B of the speaker's two decoding loops: speaker.infer_batch (the prefix form: the decoder re-reads the whole prefix for every word) against
speaker.infer_batch_cached (KV cache + one captured step replayed per word).  -> profiles/speaker_decode_ab.txt

Default configuration (hidden 512, word size 256, 3 layers, 4 heads), bf16, B = 64, T = 6, max_decode = 120, <EOS> outside the vocabulary so that both
forms run all 120 steps.  Timing: host clock around one call that ends in a device synchronise, 2 warm-up calls (the cached form captures its step in
the first), then 5 timed calls per form, the two forms alternating; median and min-max spread.  Launch counts per step: two `rocprofv3 --kernel-trace
--stats` runs per form (runs of their own, never timed), one with max_decode = 120 and one with max_decode = 1; the difference of their kernel dispatches
over calls x 119 steps leaves out the encoder, the per-call set-up and whatever else a call launches once.

    python scripts/speaker_decode_ab.py [--out profiles/speaker_decode_ab.txt]

Every GPU step is a child process under its own `timeout -k 10`; after a step that fails nothing further is started on the GPU."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, MAX_DECODE, VOCAB, FEAT = 64, 6, 120, 992, 768 + 128
WARMUP, REPS, COUNT_CALLS = 2, 5, 3


def _setup(max_decode=MAX_DECODE):
    import torch
    import vln_goat_amd
    from vln_goat_amd import speaker
    if not torch.cuda.is_available():
        raise SystemExit('speaker_decode_ab needs a GPU (no timing without one)')
    vln_goat_amd.set_compute_dtype(torch.bfloat16)
    cfg = speaker.default_config()
    torch.manual_seed(0)
    model = speaker.Transpeaker(FEAT, cfg.h_dim, cfg.wemb, VOCAB, cfg).cuda().eval()
    g = torch.Generator().manual_seed(1)
    can = torch.randn(B, T, FEAT, generator=g).cuda()
    img = torch.randn(B, T, 36, FEAT, generator=g).cuda()
    kw = dict(bos=1, eos=VOCAB + 1, pad=0, unk=3, max_decode=max_decode)        # <EOS> unreachable: every step is run
    dec = speaker.IncrementalDecoder(model, B, max_decode, T)
    forms = {'prefix': lambda: speaker.infer_batch(model, can, img, **kw),
             'cached': lambda: speaker.infer_batch_cached(model, can, img, decoder=dec, **kw)}
    return torch, forms


def measure():
    torch, forms = _setup()
    times = {k: [] for k in forms}
    for i in range(WARMUP + REPS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            words = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert words.shape == (B, MAX_DECODE + 1), words.shape
            if i >= WARMUP:
                times[name].append(dt * 1e3)
    print('RESULT ' + json.dumps(times))


def count(form, max_decode):
    torch, forms = _setup(max_decode)
    for _ in range(COUNT_CALLS):
        forms[form]()
    torch.cuda.synchronize()


def _run(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'speaker_decode_ab.txt'))
    ap.add_argument('--child', choices=['measure', 'count-prefix', 'count-cached'])
    ap.add_argument('--max-decode', type=int, default=MAX_DECODE, help='(count children) words per call')
    ap.add_argument('--no-trace', action='store_true', help='skip the four rocprofv3 runs (launch counts)')
    a = ap.parse_args()
    if a.child == 'measure':
        return measure()
    if a.child:
        return count(a.child.split('-')[1], a.max_decode)

    me = [sys.executable, os.path.abspath(__file__)]
    rc, out = _run(me + ['--child', 'measure'], 600)
    res = [ln for ln in out.splitlines() if ln.startswith('RESULT ')]
    if rc != 0 or not res:
        print(out[-4000:])
        raise SystemExit('timing step failed (exit status %d): nothing further is run on the GPU' % rc)
    times = json.loads(res[-1][7:])
    print('timing step done', flush=True)
    lines = ['speaker decoding A/B: default configuration (hidden 512, word 256, 3 layers, 4 heads), bf16, B = %d, T = %d, max_decode = %d,' % (B, T, MAX_DECODE),
             '<EOS> unreachable (both forms run all %d steps).  Wall time of one call, device-synchronised; %d warm-up calls, %d timed, forms alternating.' % (MAX_DECODE, WARMUP, REPS),
             '']
    stat = {}
    for name, label in (('prefix', 'infer_batch (prefix form)'), ('cached', 'infer_batch_cached (KV cache, replayed step)')):
        t = times[name]
        stat[name] = (statistics.median(t), min(t), max(t))
        lines.append('%-46s median %8.2f ms   min %8.2f   max %8.2f   per word %6.1f us   (%s)'
                     % (label, stat[name][0], stat[name][1], stat[name][2], 1e3 * stat[name][0] / MAX_DECODE, ', '.join('%.2f' % x for x in t)))
    ok = stat['cached'][0] < stat['prefix'][1]
    lines += ['', 'median(cached) / median(prefix) = %.3f;  acceptance (cached median below the prefix minimum): %s'
              % (stat['cached'][0] / stat['prefix'][0], 'MET' if ok else 'NOT MET')]
    trace_failed = False
    if not a.no_trace:
        lines.append('')
        for form in ('prefix', 'cached'):
            rows = {}
            for md in (MAX_DECODE, 1):
                with tempfile.TemporaryDirectory() as d:
                    rc, out = _run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--'] + me
                                   + ['--child', 'count-' + form, '--max-decode', str(md)], 600)
                    f = glob.glob(d + '/**/*kernel_stats.csv', recursive=True)
                    if rc != 0 or not f:
                        lines.append('launch count (%s, max_decode = %d): rocprofv3 run failed (exit status %d)' % (form, md, rc))
                        print(out[-3000:])
                        trace_failed = True
                        break
                    rows[md] = {r['Name']: int(r['Calls']) for r in csv.DictReader(open(f[0]))}
                    print('kernel trace (%s, max_decode = %d) done' % (form, md), flush=True)
            if trace_failed:
                break                                       # nothing further on the GPU after a failed step
            full, base = rows[MAX_DECODE], rows[1]
            steps = COUNT_CALLS * (MAX_DECODE - 1)
            per = {k: (v - base.get(k, 0)) / steps for k, v in full.items()}
            top = sorted(per.items(), key=lambda kv: -kv[1])[:6]
            lines.append('launches per step (%s): %.1f  = (%d dispatches in %d calls of %d words - %d in %d calls of 1 word) / %d steps; most frequent per step: %s'
                         % (form, (sum(full.values()) - sum(base.values())) / steps, sum(full.values()), COUNT_CALLS, MAX_DECODE, sum(base.values()),
                            COUNT_CALLS, steps, '; '.join('%s x%.1f' % (k[:48], v) for k, v in top)))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)
    if trace_failed:
        raise SystemExit(3)
    if not ok:
        raise SystemExit('the cached form is not faster than the prefix form beyond the run-to-run spread')


if __name__ == '__main__':
    main()
