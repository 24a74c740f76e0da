"""Times pre-training validation in its two forms and writes profiles/pretrain_val_ab.txt.

    python scripts/pretrain_val_ab.py [--dtype bf16] [--batches 4] [--out profiles/pretrain_val_ab.txt]

  reference-shaped   the loops of P/train_r2r_goat.py:438-583 and P/train_reverie_goat.py:587-612 as written there: torch formulas on the
                     model's `compute_loss=False` outputs, every per-batch figure read back with `.item()`.
  device             pretrain_eval.validate_mlm / _mrc / _sap / _og / _cfp: goat_val_rows / goat_val_cfp / goat_val_reduce into a float64
                     accumulator, one read per loader.

Cases: the full-size R2R and REVERIE cases of tests/helpers.CASES, a loader of `--batches` batches from different seeds, model.eval().
Two timings per task and form: `tail` runs the loop on a stand-in model that hands back outputs recorded beforehand (what the two forms
differ in), `with forward` on the real model.  Wall clock around a whole loop with a device synchronise at both ends, divided by the number
of batches; median (min .. max) of 5 after 2 warm-ups.  Device kernels per batch of the tail: torch.profiler, one loop per form.
Each case is a child process under its own `timeout -k 10`; the parent stops at the first that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_WARM, N_TIMED = 2, 5
CASE_NAMES = ('pretrain_config2_full', 'pretrain_config5_reverie_full')
LIMIT = 420


# ---- the reference-shaped loops (P/train_r2r_goat.py:438-583, P/train_reverie_goat.py:587-612; all_gather of one rank left out)
def ref_mlm(model, loader):
    import torch.nn.functional as F
    val_loss = n_correct = n_word = 0
    st = time.time()
    for batch in loader:
        scores = model(batch, task='mlm', compute_loss=False)
        labels = batch['txt_labels']
        labels = labels[labels != -1]
        val_loss += F.cross_entropy(scores, labels, reduction='sum').item()
        n_correct += (scores.max(dim=-1)[1] == labels).sum().item()
        n_word += labels.numel()
    return {'loss': val_loss / n_word, 'acc': n_correct / n_word, 'tok_per_s': n_word / (time.time() - st)}


def ref_mrc(model, loader):
    import torch.nn.functional as F
    val_loss = n_feat = tot_score = 0
    st = time.time()
    for batch in loader:
        view_logits, view_targets, _, _ = model(batch, task='mrc', compute_loss=False)
        val_loss += F.kl_div(F.log_softmax(view_logits, dim=-1), view_targets, reduction='sum').item()
        tot_score += (view_logits.max(dim=-1)[1] == view_targets.max(dim=-1)[1]).sum().item()
        n_feat += batch['vp_view_mrc_masks'].sum().item()
    return {'loss': val_loss / n_feat, 'acc': tot_score / n_feat, 'feat_per_s': n_feat / (time.time() - st)}


def ref_sap(model, loader):
    import torch
    import torch.nn.functional as F
    loss, hit, n_data = [0, 0, 0], [0, 0, 0], 0
    st = time.time()
    for batch in loader:
        gl, ll, fl, ga, la = model(batch, task='sap', compute_loss=False)
        for k, (lg, lab) in enumerate(((gl, ga), (ll, la), (fl, ga))):
            loss[k] += F.cross_entropy(lg, lab, reduction='sum').data.item()
        for k, (lg, lab) in enumerate(((gl, ga), (ll, la), (fl, ga))):
            hit[k] += torch.sum(torch.argmax(lg, 1) == lab).item()
        n_data += len(ga)
    return {'gloss': loss[0] / n_data, 'lloss': loss[1] / n_data, 'floss': loss[2] / n_data, 'gacc': hit[0] / n_data, 'lacc': hit[1] / n_data,
            'facc': hit[2] / n_data, 'tok_per_s': n_data / (time.time() - st)}


def ref_og(model, loader):
    import torch.nn.functional as F
    val_loss = n_correct = n_data = 0
    st = time.time()
    for batch in loader:
        scores = model(batch, task='og', compute_loss=False)
        labels = batch['obj_labels']
        val_loss += F.cross_entropy(scores, labels, reduction='sum').item()
        n_correct += (scores.max(dim=-1)[1] == labels).sum().item()
        n_data += labels.numel()
    return {'loss': val_loss / n_data, 'acc': n_correct / n_data, 'tok_per_s': n_data / (time.time() - st)}


def ref_cfp(model, loader, temperature):
    import torch
    import torch.nn.functional as F
    loss, hit, n_data = [0, 0, 0], [0, 0, 0], 0
    st = time.time()
    for batch in loader:
        go, vo, fo, to = model(batch, task='cfp', compute_loss=False)
        target = torch.arange(len(go)).cuda()
        sims = [(x @ to.T) / temperature for x in (go, vo, fo)]
        for k, sim in enumerate(sims):
            loss[k] += ((F.cross_entropy(sim, target, reduction='sum') + F.cross_entropy(sim.T, target, reduction='sum')) / 2.0).item()      # (the reference writes target.T: a 1-D tensor, the same)
        for k, sim in enumerate(sims):
            hit[k] += torch.sum(torch.argmax(sim, 1) == target).item()
        n_data += len(target)
    return {'gloss': loss[0] / n_data, 'lloss': loss[1] / n_data, 'floss': loss[2] / n_data, 'gacc': hit[0] / n_data, 'lacc': hit[1] / n_data,
            'facc': hit[2] / n_data, 'tok_per_s': n_data / (time.time() - st)}


def child(name, dtype, n_batches):
    import torch
    import vln_goat_amd
    from helpers import CASES, build_case, case_tasks
    from vln_goat_amd import pretrain_eval, synth

    vln_goat_amd.set_compute_dtype(torch.bfloat16 if dtype == 'bf16' else torch.float32)
    cfg, model, _ = build_case(name)
    model = model.cuda().eval()
    bkw = CASES[name][1]
    loader = [synth.batch_to(synth.make_pretrain_batch(**dict(bkw, seed=bkw['seed'] + 100 * k)), 'cuda') for k in range(n_batches)]
    tasks = case_tasks(name)
    tem = cfg.cfp_temperature

    class Replay(torch.nn.Module):
        """hands back the outputs the real model gave for this batch and task"""

        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1, device='cuda'))
            self.kept = {}

        def forward(self, batch, task, compute_loss=True):
            return self.kept[(id(batch), task)]

    replay = Replay().eval()
    with torch.no_grad():
        for batch in loader:
            for t in tasks:
                replay.kept[(id(batch), t)] = model(batch, task=t, compute_loss=False)
    forms = {'mlm': (ref_mlm, pretrain_eval.validate_mlm, ()), 'mrc': (ref_mrc, pretrain_eval.validate_mrc, ()),
             'sap': (ref_sap, pretrain_eval.validate_sap, ()), 'og': (ref_og, pretrain_eval.validate_og, ()),
             'cfp': (ref_cfp, pretrain_eval.validate_cfp, (tem,))}

    def timed(fn, m):
        out = []
        for _ in range(N_WARM + N_TIMED):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                res = fn(m, loader, *extra)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / n_batches)
        return out[N_WARM:], res

    def kernels(fn):
        """device kernels per batch of one tail loop"""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                with torch.no_grad():
                    fn(replay, loader, *extra)
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
            return n / n_batches
        except Exception as ex:                                  # (recorded as not measured, with the reason)
            return 'not measured (%s: %s)' % (type(ex).__name__, str(ex)[:80])

    res = {'case': name, 'device': torch.cuda.get_device_name(0), 'tasks': {}}
    for t in tasks:
        ref, new, extra = forms[t]
        r = {}
        r['ref_tail'], ref_log = timed(ref, replay)
        r['new_tail'], new_log = timed(new, replay)
        r['ref_full'], _ = timed(ref, model)
        r['new_full'], _ = timed(new, model)
        r['ref_kernels'], r['new_kernels'] = kernels(ref), kernels(new)
        r['max_diff'] = max(abs(ref_log[k] - new_log[k]) for k in ref_log if not k.endswith('_per_s'))
        r['rows'] = sum(int(replay.kept[(id(b), 'mlm')].shape[0]) for b in loader) / n_batches if t == 'mlm' else None
        r['log'] = {k: v for k, v in new_log.items() if not k.endswith('_per_s')}
        res['tasks'][t] = r
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', choices=('bf16', 'f32'), default='bf16')
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pretrain_val_ab.txt'))
    ap.add_argument('--child', choices=CASE_NAMES)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.dtype, args.batches)
    got = []
    for name in CASE_NAMES:           # every case a fresh child under its own time limit; nothing more is started after one that fails
        cmd = ['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__), '--child', name, '--dtype', args.dtype,
               '--batches', str(args.batches)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit('%s ended with status %d: nothing further is run' % (name, r.returncode))
        got.append(json.loads(r.stdout.strip().splitlines()[-1]))
    fmt = lambda t: '%8.3f ms (%.3f .. %.3f)' % (statistics.median(t), min(t), max(t))
    kfmt = lambda k: ('%.1f' % k) if isinstance(k, float) else str(k)
    lines = ['pre-training validation: the reference-shaped loops (torch formulas, .item() per figure) against pretrain_eval.validate_* (scripts/pretrain_val_ab.py)',
             'device: %s   compute dtype %s   one run on one box' % (got[0]['device'], args.dtype),
             'per BATCH: wall clock of a loop over %d batches, synchronised at both ends, over %d; median of %d after %d warm-ups (min .. max); each case in a process of its own' % (
                 args.batches, args.batches, N_TIMED, N_WARM),
             'tail = the loop on recorded compute_loss=False outputs (what the two forms differ in); with forward = on the real model in eval mode',
             'kernels = device kernels per batch of the tail (torch.profiler, copies not counted; a fraction is a once-per-loader kernel, the zero fill of the accumulator, shared out over the batches)', '']
    for g in got:
        lines.append('%s' % g['case'])
        for t, r in g['tasks'].items():
            lines += ['  %s%s' % (t, '   (%.0f masked rows x 50265 per batch)' % r['rows'] if r.get('rows') else ''),
                      '    tail          reference-shaped %s   kernels %s' % (fmt(r['ref_tail']), kfmt(r['ref_kernels'])),
                      '    tail          device           %s   kernels %s' % (fmt(r['new_tail']), kfmt(r['new_kernels'])),
                      '    with forward  reference-shaped %s' % fmt(r['ref_full']),
                      '    with forward  device           %s' % fmt(r['new_full']),
                      '    largest |reference-shaped - device| over the loss / accuracy keys: %.3e' % r['max_diff']]
        lines.append('')
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
