"""Regenerates tests/golden/backtranslate_shrink.json: rows of speaker word ids with what the reference's own `Tokenizer.shrink` and
`Tokenizer.decode_sentence` (map_nav_src/utils/data.py) make of them — the host half of the back-translation rollout
(map_nav_src/r2r/agent.py:457-474) that speaker.shrink_words / decode_words and goat_retok_rows restate.

    python tests/golden/make_golden_backtranslate.py          (CPU; needs the reference tree, see ref_shim.py)

utils/data.py imports packages at module level that `shrink` never touches (nltk, spacy, sklearnex, ...); those that are not installed
are stubbed in sys.modules before the import, as ref_shim.py stubs pynvml.  Only data is written: vocabularies, rows and results.

Two vocabularies.  'small' is <PAD> <UNK> <EOS> a b c d (+ <BOS> = 7, which the reference's Tokenizer appends): the hand-written rows,
every quirk once.  'rich' has punctuation, '..', digits, mixed alphanumerics, an apostrophe word, an underscore word and words that
look like the special tokens: seeded random rows at the widths where goat_retok_rows changes its course (2, 3, a wave, a block of
threads, the 512 limit and their neighbours), with runs that straddle columns 63 / 64 and 255 / 256.  A row the reference raises on
(everything collapses: np.argmax of an empty list) is recorded with "raises": true.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = ['<PAD>', '<UNK>', '<EOS>', 'a', 'b', 'c', 'd']
RICH = ['<PAD>', '<UNK>', '<EOS>', 'walk', 'turn', 'left', 'right', 'the', 'stairs', 'door', ',', '.', '..', '!', '?', "'", "don't", '2',
        '42', 'room2', '2nd', 'b4', 'wait_here', '_', 'eos', '<eos', 'EOS>', 'bos', 'up', 'down', 'past', 'a', 'an', 'kitchen', 'go', 'stop',
        'and', 'then', 'walking', 'wal']
WIDTHS = (2, 3, 63, 64, 65, 121, 256, 257, 512)


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return lambda *a, **k: None


def import_reference_tokenizer():
    sys.path.insert(0, HERE)
    import ref_shim
    for name in ('jsonlines', 'h5py', 'networkx', 'spacy', 'nltk', 'transformers', 'sklearnex', 'sklearn', 'sklearn.cluster', 'joblib'):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    p = ref_shim.REF_ROOT + '/map_nav_src'
    if p not in sys.path:
        sys.path.insert(0, p)
    from utils.data import Tokenizer
    return Tokenizer


def hand_rows():
    B, E, P = 7, 2, 0
    return [[B, 3, 4, 4, E, P, P], [B, 3, E], [B, 3, 4, 5], [B, E], [B, E, P], [B, 3, P, 4, E, P], [E, 3, 4, P],
            [B, B, 3, 4, E, P], [B, B, B, E, P, P], [B, 3, 4, E, E, P], [B, 3, E, E], [B, 3, E, 4, E, P, P], [3, 4, E, P], [3, B, 4, E, P],
            [B, 3, 3, 3, E, P], [B, P, 3, E, P], [B, 3, 4, P], [B, 1, 3, E, P, P], [B, 3, 4, 5, 6, 5, 4, E],
            [B, B], [3, 3, 3], [P, P], [B]]


def random_rows(rs, V, bos, eos, pad):
    rows = []
    word = lambda: int(rs.randint(3, V + 1))          # any word, <BOS> included
    for width in WIDTHS:
        for kind in range(5):
            n = width if kind in (1, 2) else int(rs.randint(1, width + 1))          # columns before the <PAD> tail
            row = [bos]
            while len(row) < n:
                w = word()
                run = int(rs.choice([1, 1, 1, 2, 3, 5])) if kind != 2 else int(rs.choice([1, 2, 4, 9]))
                row += [w] * run
            row = row[:n]
            if kind == 0 and n >= 2:                    # sentence, <EOS>, <PAD> tail
                row[-1] = eos
            elif kind == 3 and n >= 4:                  # a <PAD> inside the sentence, <EOS> behind it
                row[int(rs.randint(1, n - 1))] = pad
                row[-1] = eos
            elif kind == 4 and n >= 3:                  # two <EOS>: the first one counts
                row[int(rs.randint(1, n - 1))] = eos
                row[-1] = eos
            row += [pad] * (width - len(row))
            if kind == 2:                               # runs across the wave and the thread-block boundaries
                for lo in (62, 254):
                    if width >= lo + 4:
                        row[lo:lo + 4] = [row[lo]] * 4
            rows.append(row)
    return rows


def results(tok, rows):
    out = []
    for row in rows:
        try:
            kept = [int(w) for w in tok.shrink(list(row))]
        except ValueError:
            out.append({'row': row, 'raises': True})
            continue
        out.append({'row': row, 'shrink': kept, 'sentence': tok.decode_sentence(kept)})
    return out


def main():
    Tokenizer = import_reference_tokenizer()
    cases = []
    for name, vocab, make in (('small', SMALL, lambda t: hand_rows()),
                              ('rich', RICH, lambda t: random_rows(np.random.RandomState(20), len(RICH), len(RICH), 2, 0))):
        tok = Tokenizer(vocab=list(vocab), encoding_length=80)
        bos, eos, pad = tok.word_to_index['<BOS>'], tok.word_to_index['<EOS>'], tok.word_to_index['<PAD>']
        assert (bos, eos, pad) == (len(vocab), 2, 0)
        words = [tok.index_to_word[i] for i in range(tok.vocab_size())]
        cases.append({'name': name, 'vocab': words, 'bos': bos, 'eos': eos, 'pad': pad, 'unk': tok.word_to_index['<UNK>'], 'rows': results(tok, make(tok))})
    table = {(7, 3, 4, 4, 2, 0, 0): 'a b', (7, 3, 2): 'a', (7, 3, 4, 5): 'a b', (7, 2): '<BOS>', (7, 2, 0): '', (7, 3, 0, 4, 2, 0): 'a', (2, 3, 4, 0): '<EOS> a b'}
    got = {tuple(r['row']): r.get('sentence') for r in cases[0]['rows']}
    for row, want in table.items():
        assert got[row] == want, (row, got[row], want)
    path = os.path.join(HERE, 'backtranslate_shrink.json')
    with open(path, 'w') as f:
        json.dump({'cases': cases}, f, separators=(',', ':'))
    print('wrote', path, os.path.getsize(path), 'bytes;', [(c['name'], len(c['rows']), sum(bool(r.get('raises')) for r in c['rows'])) for c in cases])


if __name__ == '__main__':
    main()
