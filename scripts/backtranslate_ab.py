"""A/B of the speaker -> instruction step of the back-translation rollout: the host way (read the decoded words back, `shrink` /
`decode_sentence` / a tokenizer call per sentence in Python, upload txt_ids / txt_masks) against speaker.BackTranslator (one
goat_retok_rows launch into the same buffers).  -> profiles/backtranslate_ab.txt

Default speaker configuration (hidden 512, word 256, 3 layers, 4 heads), bf16, B = 12, T = 6, max_decode = 120, a vocabulary of 992
pseudo-words and a byte-level BPE with RoBERTa's pre-tokenisation trained over it with `tokenizers` (no tokenizer files are shipped).
The speaker is untrained (and its always-on attention dropout is off, so that both forms decode the same words): its rows rarely end, so a row holds up to 120 words — the long end of what the step sees.

Two figures per form, both wall time that ends in a device synchronise, median of 5 after 2 warm-ups, the forms alternating:
  whole   encoder + decode loop + the words-to-instruction step;
  step    the words-to-instruction step alone, on the words the decode loop has just left in the decoder state.

    python scripts/backtranslate_ab.py [--out profiles/backtranslate_ab.txt]

The measurement is one child process under its own `timeout -k 10`."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, MAX_DECODE, VOCAB, FEAT, L = 12, 6, 120, 992, 768 + 128, 200
WARMUP, REPS = 2, 5
PAD, UNK, EOS, AGENT_BOS, AGENT_EOS = 0, 1, 2, 0, 2


def _vocab():
    import numpy as np
    rs = np.random.RandomState(0)
    syl = ['wa', 'lk', 'tu', 'rn', 'le', 'ft', 'ri', 'ght', 'sta', 'irs', 'do', 'or', 'ro', 'om', 'ki', 'tch', 'en', 'pa', 'st', 'go', 'up', 'ba', 'th']
    words, seen = ['<PAD>', '<UNK>', '<EOS>', ',', '.'], set()
    while len(words) < VOCAB - 1:
        w = ''.join(syl[i] for i in rs.randint(0, len(syl), rs.randint(1, 4)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words + ['<BOS>']


def _encode(vocab):
    import numpy as np
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers
    rs = np.random.RandomState(1)
    corpus = [' '.join(vocab[i] for i in rs.randint(1, len(vocab), 12)) for _ in range(2000)]
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    tok.train_from_iterator(corpus, trainers.BpeTrainer(vocab_size=600, special_tokens=['<s>', '<pad>', '</s>'],
                                                        initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False))
    return lambda s: tok.encode(s, add_special_tokens=False).ids


def measure():
    import torch
    import vln_goat_amd
    from vln_goat_amd import speaker
    if not torch.cuda.is_available():
        raise SystemExit('backtranslate_ab needs a GPU (no timing without one)')
    vln_goat_amd.set_compute_dtype(torch.bfloat16)
    vocab = _vocab()
    bos = len(vocab) - 1
    encode = _encode(vocab)
    table = speaker.RetokTable.build(vocab, encode, device='cuda')
    cfg = speaker.default_config(attn_dropout_always=False)      # (the always-on attention dropout would make every decode a new draw)
    torch.manual_seed(0)
    model = speaker.Transpeaker(FEAT, cfg.h_dim, cfg.wemb, len(vocab), cfg).cuda().eval()
    g = torch.Generator().manual_seed(1)
    can = torch.randn(B, T, FEAT, generator=g).cuda()
    img = torch.randn(B, T, 36, FEAT, generator=g).cuda()
    bt = speaker.BackTranslator(model, table, B, MAX_DECODE, T, bos, EOS, PAD, UNK, AGENT_BOS, AGENT_EOS)
    ids_dev = torch.zeros(B, L, dtype=torch.int64, device='cuda')
    masks_dev = torch.zeros(B, L, dtype=torch.bool, device='cuda')
    ids_host = torch.zeros(B, L, dtype=torch.int64).pin_memory()
    masks_host = torch.zeros(B, L, dtype=torch.bool).pin_memory()
    kw = dict(bos=bos, eos=EOS, pad=PAD, unk=UNK, max_decode=MAX_DECODE)

    def host_step(words):
        rows = words.cpu().tolist()
        ids_host.zero_()
        masks_host.zero_()
        for i, row in enumerate(rows):
            text = table.sentence(speaker.decode_words(speaker.shrink_words(row, bos, EOS), PAD))
            enc = ([AGENT_BOS] + encode(text) + [AGENT_EOS])[:L]
            ids_host[i, :len(enc)] = torch.tensor(enc, dtype=torch.int64)
            masks_host[i, :len(enc)] = True
        ids_dev.copy_(ids_host, non_blocking=True)
        masks_dev.copy_(masks_host, non_blocking=True)

    def device_step():
        st = bt.decoder.state
        vln_goat_amd.hipops.retok_rows(st.words, table, ids_dev, masks_dev, bos, EOS, PAD, AGENT_BOS, AGENT_EOS, 0, L, state=st, lens=bt.lens,
                                       status=bt.status, check=False)
        vln_goat_amd.layers.refresh_masks(only=[masks_dev, ids_dev], force=True)

    def host_whole():
        host_step(speaker.infer_batch_cached(model, can, img, decoder=bt.decoder, already_dropfeat=True, **kw))

    def device_whole():
        bt.run(can, img, ids_dev, masks_dev)

    def cut():
        st = bt.decoder.state
        n = MAX_DECODE + 1 if int(st.n_live.item()) else int(st.end_step.max().item()) + 2
        return st.words[:, :n].clone()

    times = {k: [] for k in ('host whole', 'device whole', 'host step', 'device step')}
    info = {}
    for i in range(WARMUP + REPS):
        for name, fn in (('host whole', host_whole), ('device whole', device_whole)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
            got = (ids_dev.cpu(), masks_dev.cpu())
            if name == 'host whole':
                want = got
            else:
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), 'the two forms disagree'
        # the step alone, on the state the last decode left
        for name in ('host step', 'device step'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == 'host step':
                host_step(cut())
            else:
                device_step()
            torch.cuda.synchronize()
            if i >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
        info = {'columns': int(cut().shape[1]), 'tokens': masks_dev.sum(1).tolist()}
    print('RESULT ' + json.dumps({'times': times, 'info': info}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'backtranslate_ab.txt'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return measure()
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--child'], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    res = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    if r.returncode != 0 or not res:
        print(r.stdout[-4000:])
        raise SystemExit('timing step failed (exit status %d)' % r.returncode)
    d = json.loads(res[-1][7:])
    lines = ['back-translation A/B: speaker words -> agent instruction.  Default speaker (hidden 512, word 256, 3 layers, 4 heads), bf16, B = %d, T = %d,' % (B, T),
             'max_decode = %d, vocabulary %d, text bucket %d.  Wall time ending in a device synchronise; %d warm-ups, %d timed, forms alternating.' % (MAX_DECODE, VOCAB, L, WARMUP, REPS),
             'The decoded rows were %d columns wide; instruction lengths %s tokens.  Both forms wrote identical txt_ids / txt_masks.' % (d['info']['columns'], d['info']['tokens']),
             '']
    med = {}
    for name, label in (('host whole', 'whole, host: decode + read-back + Python shrink / decode / tokenise + upload'),
                        ('device whole', 'whole, device: BackTranslator.run'),
                        ('host step', 'step alone, host: read-back + Python + upload'),
                        ('device step', 'step alone, device: goat_retok_rows + mask refresh')):
        t = d['times'][name]
        med[name] = statistics.median(t)
        lines.append('%-84s median %9.3f ms   min %9.3f   max %9.3f   (%s)' % (label, med[name], min(t), max(t), ', '.join('%.3f' % x for x in t)))
    lines += ['', 'step alone: host / device = %.1f;  whole: host - device = %.3f ms of %.3f ms' % (
        med['host step'] / med['device step'], med['host whole'] - med['device whole'], med['host whole'])]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
