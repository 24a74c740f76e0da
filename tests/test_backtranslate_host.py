"""The host half of back-translation (speaker.shrink_words / decode_words / RetokTable), no GPU: equal to the reference's own
`Tokenizer.shrink` / `decode_sentence` on every row of tests/golden/backtranslate_shrink.json (made by make_golden_backtranslate.py
from the reference class), and the per-word table equal to whole-sentence tokenisation by a byte-level BPE with RoBERTa's
pre-tokenisation that is trained here from an in-memory corpus."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    with open(os.path.join(HERE, 'golden', 'backtranslate_shrink.json')) as f:
        return json.load(f)['cases']


_BPE = {}


def bpe_encode(vocab):
    """str -> ids without special tokens, of a byte-level BPE trained on sentences over `vocab` (cached per vocabulary)"""
    key = tuple(vocab)
    if key not in _BPE:
        from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
        rs = np.random.RandomState(7)
        words = [w for w in vocab if w not in ('<PAD>',)]
        corpus = [' '.join(words[i] for i in rs.randint(0, len(words), rs.randint(3, 12))) for _ in range(400)]
        tok = Tokenizer(models.BPE())
        tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
        tok.decoder = decoders.ByteLevel()
        tok.train_from_iterator(corpus, trainers.BpeTrainer(vocab_size=330, special_tokens=['<s>', '<pad>', '</s>'],
                                                            initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False))
        _BPE[key] = lambda s: tok.encode(s, add_special_tokens=False).ids
    return _BPE[key]


def test_the_golden_file_holds_the_cases_the_reference_was_run_on():
    small = {tuple(r['row']): r.get('sentence') for r in golden()[0]['rows']}
    table = {(7, 3, 4, 4, 2, 0, 0): 'a b', (7, 3, 2): 'a', (7, 3, 4, 5): 'a b', (7, 2): '<BOS>', (7, 2, 0): '', (7, 3, 0, 4, 2, 0): 'a',
             (2, 3, 4, 0): '<EOS> a b'}
    for row, want in table.items():
        assert small[row] == want, row
    rich = golden()[1]
    assert sorted({len(r['row']) for r in rich['rows']}) == [2, 3, 63, 64, 65, 121, 256, 257, 512]
    assert any(len(r['row']) == 512 and len(set(r['row'][254:258])) == 1 and len(set(r['row'][62:66])) == 1 for r in rich['rows'])


def test_shrink_and_decode_equal_the_reference_on_every_golden_row():
    from vln_goat_amd import speaker
    n = 0
    for case in golden():
        bos, eos, pad, vocab = case['bos'], case['eos'], case['pad'], case['vocab']
        for r in case['rows']:
            if r.get('raises'):
                with pytest.raises(ValueError):
                    speaker.shrink_words(r['row'], bos, eos)
                continue
            kept = speaker.shrink_words(r['row'], bos, eos)
            assert kept == r['shrink'], r['row']
            assert ' '.join(vocab[w] for w in speaker.decode_words(kept, pad)) == r['sentence'], r['row']
            n += 1
    assert n >= 60


def test_a_one_column_row_raises_and_an_empty_one_is_empty():
    from vln_goat_amd import speaker
    with pytest.raises(ValueError):
        speaker.shrink_words([7], 7, 2)
    with pytest.raises(ValueError):
        speaker.shrink_words([2], 7, 2)
    assert speaker.shrink_words([], 7, 2) == []


def test_table_expansion_equals_whole_sentence_tokenisation():
    from vln_goat_amd import speaker
    case = golden()[1]
    vocab, bos, eos, pad = case['vocab'], case['bos'], case['eos'], case['pad']
    encode = bpe_encode(vocab)
    table = speaker.RetokTable.build(vocab, encode, device='cpu')
    assert table.V == len(vocab) and table.first_start.numel() == table.V + 1 and table.rest_start.numel() == table.V + 1
    assert int(table.first_start[-1]) == sum(len(x) for x in table.first) and int(table.rest_start[-1]) == table.rest_ids.numel()
    assert any(table.first[w] != table.rest[w] for w in range(table.V))          # "walk" and " walk" differ
    sentences = [speaker.decode_words(r['shrink'], pad) for r in case['rows'] if not r.get('raises')]
    rs = np.random.RandomState(3)
    sentences += [[int(w) for w in rs.randint(1, len(vocab), rs.randint(2, 30))] for _ in range(1000)]
    n = 0
    for words in sentences:
        text = ' '.join(vocab[w] for w in words)
        assert table.host(words) == encode(text), text
        n += len(words) > 1
    assert n >= 1000
    table.check(encode, sentences)
    for r in case['rows']:
        if not r.get('raises'):
            assert table.sentence(speaker.decode_words(r['shrink'], pad)) == r['sentence']


def test_check_raises_for_an_encode_that_merges_across_words():
    from vln_goat_amd import speaker
    vocab = ['<PAD>', '<UNK>', '<EOS>', 'go', 'up', 'stairs', '<BOS>']
    ids = {}

    def merging(s):
        """one id per distinct string, but 'go up' becomes a single token"""
        out = []
        for piece in s.replace('go up', 'go_up').split(' '):
            if piece:
                out.append(ids.setdefault(piece, len(ids) + 10))
        return out
    table = speaker.RetokTable.build(vocab, merging, device='cpu')
    table.check(merging, [[3, 5], [4, 3], [5]])
    with pytest.raises(ValueError, match='merges'):
        table.check(merging, [[5, 3, 4]])


def test_max_len_is_a_plain_slice_that_can_lose_the_closing_token():
    from vln_goat_amd import speaker
    vocab = ['<PAD>', '<UNK>', '<EOS>', 'a', 'b', 'c', 'd', '<BOS>']
    first = [[], [900], [901], [10], [20, 21], [30, 31, 32], [], [902]]
    rest = [[], [900], [901], [11], [22, 23], [33, 34, 35], [], [902]]
    table = speaker.RetokTable(vocab, first, rest, device='cpu')
    row = [7, 3, 4, 6, 5, 2, 0, 0]                      # a b d c: 1 + 2 + 0 + 3 = 6 ids, 8 tokens with <s> and </s>
    full = [0, 10, 22, 23, 33, 34, 35, 2]
    enc = lambda n: table.instr_encoding(row, 7, 2, 0, agent_bos=0, agent_eos=2, max_len=n)
    assert enc(None) == full
    assert enc(9) == full                                # max_len - 1 tokens: untouched
    assert enc(8) == full                                # exactly max_len
    assert enc(7) == full[:7] and enc(7)[-1] == 35       # max_len + 1: the </s> is lost
    assert enc(5) == [0, 10, 22, 23, 33]                 # cut inside a word's ids
    assert table.host([6]) == [] and table.instr_encoding([7, 6, 2], 7, 2, 0, 0, 2) == [0, 2]
