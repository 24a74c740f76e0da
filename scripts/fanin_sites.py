"""Which tensors of a step make the autograd ENGINE launch gradient additions?  A tensor with k consumers costs k - 1 `add` launches in
the backward pass.  Walks the autograd graph of one forward per task, counts the incoming edges of every (node, output slot) and prints the
ones with more than one, with the Python line that created the node (anomaly-mode traceback).
    python scripts/fanin_sites.py [pretrain|nav]"""
import os, sys, collections
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
import vln_goat_amd
from vln_goat_amd import config as gcfg, pretrain_model, synth, hipops

torch.cuda.set_device(0)
torch.autograd.set_detect_anomaly(True, check_nan=False)
cfg = gcfg.make_config(num_l_layers=2, num_top_layer=3, num_pano_layers=2, vocab_size=1000)
torch.manual_seed(0)
model = pretrain_model.GlocalTextPathCMTPreTraining(cfg).cuda().train()
vln_goat_amd.set_compute_dtype(torch.bfloat16)
gb = synth.batch_to(synth.make_pretrain_batch(B=4, T=3, L=20, seed=50, vocab_size=1000, style='survey'), 'cuda')
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def site(node):
    tb = node.metadata.get('traceback_') if hasattr(node, 'metadata') else None
    if not tb:
        return '?'
    frames = []
    for line in tb:
        for l in line.splitlines():
            l = l.strip()
            if l.startswith('File') and ROOT in l and 'fanin_sites' not in l:
                frames.append(l.replace(ROOT + '/', '').replace('File ', '').replace('"', ''))
    outer = [f for f in frames if 'hipops.py' not in f and '/ops_' not in f]      # (the op layer: the facade and the family modules behind it)
    return ' <- '.join(([frames[-1]] if frames else ['?']) + outer[-2:][::-1])


for task in ('mlm', 'sap', 'cfp'):
    loss = model(gb, task, compute_loss=True).mean()
    indeg = collections.Counter()
    seen, stack = set(), [loss.grad_fn]
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        for nxt, slot in n.next_functions:
            if nxt is not None:
                indeg[(nxt, slot)] += 1
                stack.append(nxt)
    rows = collections.Counter()
    for (n, slot), k in indeg.items():
        if k > 1 and 'AccumulateGrad' not in n.name():
            rows[(n.name(), slot, site(n))] += k - 1
    print('== %s: %d engine additions' % (task, sum(rows.values())))
    for (name, slot, where), k in rows.most_common():
        print('  %3d  %-28s out %d  %s' % (k, name, slot, where))
    acc = sum(k - 1 for (n, slot), k in indeg.items() if k > 1 and 'AccumulateGrad' in n.name())
    print('  (+ %d in-place accumulations into parameter gradients: a parameter used more than once)' % acc)
    del loss
