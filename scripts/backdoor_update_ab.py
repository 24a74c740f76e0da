"""Times backdoor.InstrDictionaries.update against the host form of update_z_dict and writes profiles/backdoor_update_ab.txt.

    python scripts/backdoor_update_ab.py [--instructions 2048] [--tokens 80] [--layers 9] [--dtype bf16] [--out profiles/backdoor_update_ab.txt]

Both forms make the same model calls (mode='instr_zdict_update', batches of 64, the current dictionaries as inputs).  The device form adds
the picked rows with goat_dict_accumulate and ends with goat_dict_finish; the host form does what M/r2r/agent.py:769-826 does: the
batch output .float().cpu(), one numpy row appended per picked token, np.mean per key, the results uploaded.  The token walk is done
once for both (the reference repeats it in every update, which is not charged to the host form here).  The two forms alternate; wall
clock around each call with a device synchronise at both ends, median (min .. max) of 5 after 2 warm-ups each.  The largest difference
between the two forms' features is printed with the largest feature magnitude.
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vln_goat_amd  # noqa: E402
from vln_goat_amd import backdoor, nav_model, synth  # noqa: E402

N_LANDMARKS, N_DIRECTIONS = 40, 30


def instructions(n, n_tok, vocab, seed=0):
    rs = np.random.RandomState(seed)
    data = []
    for i in range(n):
        toks = ['##x' if (j > 0 and rs.rand() < 0.1) else 'w' for j in range(n_tok - 2)]
        words = sum(t[0] != '#' for t in toks)
        lm = [(w, 'landmark%d' % rs.randint(N_LANDMARKS)) for w in range(words) if rs.rand() < 0.15]
        di = [(w, 'direction%d' % rs.randint(N_DIRECTIONS)) for w in range(words) if rs.rand() < 0.1]
        data.append({'instr_id': str(i), 'instr_encoding': [0] + [int(v) for v in rs.randint(4, vocab, n_tok - 2)] + [2], 'tokens': toks,
                     'words': (lm, di)})
    return data


def host_update(model, plan, picks, current, device):
    """The host form.  picks: per batch [(b, pos, kind, key)].  current: None or {kind: (feats [K, H], pzs [K])} on the device."""
    lists = {k: {} for k in backdoor.KINDS}
    was = model.training
    model.eval()
    for batch, batch_picks in zip(plan.batches, picks):
        inputs = {'z_txt': batch.ids.to(device), 'z_txt_mask': batch.mask.to(device), 'front_txt_feats': None}
        for kind in backdoor.KINDS:
            f, p = current[kind] if current is not None else (None, None)
            inputs['instr_z_%s_features' % kind] = None if f is None else f.repeat(batch.size, 1).reshape(batch.size, -1, f.shape[1])
            inputs['instr_z_%s_pzs' % kind] = None if p is None else p.repeat(batch.size, 1).reshape(batch.size, -1, 1)
        with torch.no_grad():
            out = model('instr_zdict_update', inputs).detach().float().cpu()
        for b, pos, kind, key in batch_picks:
            lists[kind].setdefault(key, []).append(np.array(out[b][pos]))
    res = {}
    for kind in backdoor.KINDS:
        total = sum(len(v) for v in lists[kind].values())
        feats = np.array([np.mean(np.array(v), axis=0) for v in lists[kind].values()])
        pzs = np.array([len(v) / total for v in lists[kind].values()])
        res[kind] = (torch.from_numpy(feats).to(device), torch.from_numpy(pzs).to(device).float())
    model.train(was)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instructions', type=int, default=2048)
    ap.add_argument('--tokens', type=int, default=80)
    ap.add_argument('--layers', type=int, default=9)
    ap.add_argument('--vocab', type=int, default=50265)
    ap.add_argument('--dtype', choices=('bf16', 'f32'), default='bf16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'backdoor_update_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('backdoor_update_ab.py measures on the GPU: none found')
    device = torch.device('cuda')
    vln_goat_amd.set_compute_dtype(torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    cfg = nav_model.nav_config_from_args(SimpleNamespace(num_l_layers=args.layers, num_x_layers=1, num_pano_layers=1, vocab_size=args.vocab,
                                                          do_back_txt=True, do_back_txt_type='type_2', mode='train'))
    model = nav_model.GlocalTextPathNavCMT(cfg)
    model.load_state_dict(synth.seeded_state_dict(model, seed=11))
    model = model.to(device).train()
    data = instructions(args.instructions, args.tokens, args.vocab)
    plan = backdoor.InstrPickPlan(data, lambda it: it['tokens'], lambda it: it['words'])
    picks = []
    for i0 in range(0, len(data), plan.batch_size):
        picks.append([(b, pos, kind, key) for b, it in enumerate(data[i0:i0 + plan.batch_size])
                      for pos, kind, key in backdoor.pick_positions(it['tokens'], *it['words'])])
    dicts = backdoor.InstrDictionaries(device)
    dicts.update(model, plan)                                  # both forms start from dictionaries that exist
    start = {k: (dicts.feats[k].clone(), dicts.pzs[k].clone()) for k in backdoor.KINDS}
    state = {}

    def device_form():
        for k in backdoor.KINDS:
            dicts.feats[k].copy_(start[k][0])
            dicts.pzs[k].copy_(start[k][1])
        dicts.update(model, plan)

    def host_form():
        state['host'] = host_update(model, plan, picks, start, device)

    times = {'device': [], 'host': []}
    for i in range(7):
        for name, fn in (('device', device_form), ('host', host_form)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    diff = max(float((dicts.feats[k] - state['host'][k][0]).abs().max()) for k in backdoor.KINDS)
    peak = max(float(dicts.feats[k].abs().max()) for k in backdoor.KINDS)
    n_picks = {k: sum(plan.counts[k].values()) for k in backdoor.KINDS}
    lines = ['update_z_dict, device form against host form (scripts/backdoor_update_ab.py)',
             'device: %s   %d instructions of %d tokens, %d batches of %d, %d text layers, compute dtype %s'
             % (torch.cuda.get_device_name(0), args.instructions, args.tokens, len(plan.batches), plan.batch_size, args.layers, args.dtype),
             'picks: %d landmark rows over %d keys, %d direction rows over %d keys'
             % (n_picks['landmark'], len(plan.keys['landmark']), n_picks['direction'], len(plan.keys['direction'])),
             'wall clock per update, synchronised, the two forms alternating, median of 5 after 2 warm-ups (min .. max); one run on one box', '']
    for name, label in (('device', 'InstrDictionaries.update (goat_dict_accumulate / goat_dict_finish)'),
                        ('host', 'host form (.float().cpu(), numpy appends, np.mean)')):
        t = times[name]
        lines.append('%-70s %9.2f ms (%.2f .. %.2f)' % (label, statistics.median(t), min(t), max(t)))
    lines.append('')
    lines.append('largest |device - host| over all features: %.3e (largest |feature| %.3f)' % (diff, peak))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
