"""Back-translation on the device: goat_retok_rows against the host pipeline (speaker.shrink_words -> decode_words -> RetokTable.host,
themselves pinned to the reference by tests/test_backtranslate_host.py) and goat_scale_cols against torch, both with torch.equal —
integers, and one float32 multiply rounded once; then the wiring: VLNBert('panorama') with `env_noise`, BackTranslator.run, and a
device walk on the instruction a kernel wrote."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda'
AGENT_BOS, AGENT_EOS = 0, 2


def _golden():
    with open(os.path.join(HERE, 'golden', 'backtranslate_shrink.json')) as f:
        return json.load(f)['cases']


_CACHE = {}


def _bpe_table(case):
    """the RetokTable of a byte-level BPE trained over the case's vocabulary (test_backtranslate_host.bpe_encode), on the GPU"""
    if case['name'] not in _CACHE:
        from test_backtranslate_host import bpe_encode
        from vln_goat_amd import speaker
        _CACHE[case['name']] = speaker.RetokTable.build(case['vocab'], bpe_encode(case['vocab']), device=DEV)
    return _CACHE[case['name']]


def _synthetic_table(V):
    """words of 0, 1 and 6 ids (and everything between), different at the start of a sentence and behind a space"""
    from vln_goat_amd import speaker
    n_first = [(3 * w) % 7 for w in range(V)]
    n_rest = [(5 * w + 1) % 7 for w in range(V)]
    first = [[1000 + 10 * w + j for j in range(n)] for w, n in enumerate(n_first)]
    rest = [[2000 + 10 * w + j for j in range(n)] for w, n in enumerate(n_rest)]
    assert {0, 1, 6} <= set(n_first) and {0, 1, 6} <= set(n_rest)
    return speaker.RetokTable(['w%d' % w for w in range(V)], first, rest, device=DEV)


def _expected(table, rows, case, max_len, ldo, fill):
    ids = torch.full((len(rows), ldo), fill, dtype=torch.int64)
    mask = torch.zeros(len(rows), ldo, dtype=torch.bool)
    lens = torch.zeros(len(rows), dtype=torch.int32)
    for i, row in enumerate(rows):
        enc = table.instr_encoding(row, case['bos'], case['eos'], case['pad'], AGENT_BOS, AGENT_EOS, max_len)
        ids[i, :len(enc)] = torch.tensor(enc, dtype=torch.int64)
        mask[i, :len(enc)] = True
        lens[i] = len(enc)
    return ids, mask, lens


def _run(table, rows, case, width, ldw, max_len, ldo, fill, **kw):
    from vln_goat_amd import hipops
    words = torch.full((len(rows), ldw), case['pad'], dtype=torch.int64)
    for i, row in enumerate(rows):
        words[i, :len(row)] = torch.tensor(row, dtype=torch.int64)
    out_ids = torch.full((len(rows), ldo), 777, dtype=torch.int64, device=DEV)          # (stale contents: every slot must be written)
    out_masks = torch.ones(len(rows), ldo, dtype=torch.bool, device=DEV)
    lens = hipops.retok_rows(words.to(DEV), table, out_ids, out_masks, case['bos'], case['eos'], case['pad'], AGENT_BOS, AGENT_EOS, fill,
                             max_len, width=width, **kw)
    return out_ids.cpu(), out_masks.cpu(), lens.cpu()


def _check(got, want, tag):
    for g, w, name in zip(got, want, ('ids', 'mask', 'lens')):
        assert g.dtype == w.dtype and torch.equal(g, w), (tag, name, g, w)


@pytest.mark.parametrize('which', ['small', 'rich'])
def test_retok_rows_equals_the_host_pipeline_on_every_golden_row(which):
    case = [c for c in _golden() if c['name'] == which][0]
    tables = [_synthetic_table(len(case['vocab']))] + ([_bpe_table(case)] if which == 'rich' else [])
    by_width = {}
    for r in case['rows']:
        if not r.get('raises'):
            by_width.setdefault(len(r['row']), []).append(r['row'])
    n = 0
    for width, rows in sorted(by_width.items()):
        for table in tables:
            for B in (1, 3, 17):
                batch = [rows[(n + i) % len(rows)] for i in range(B)]
                ldw = width if B == 3 else min(512, width + 5)          # columns behind `width` are never read
                ldo = 40 if B == 1 else 600                             # short rows cut long sentences, long rows hold them whole
                max_len = min(ldo - (3 if B == 17 else 0), 512)
                want = _expected(table, batch, case, max_len, ldo, 1)
                _check(_run(table, batch, case, width, ldw, max_len, ldo, 1), want, (width, B))
                n += 1
    assert n >= 9


def test_retok_rows_max_len_is_a_plain_slice():
    from vln_goat_amd import speaker
    case = dict(bos=7, eos=2, pad=0)
    first = [[], [900], [901], [10], [20, 21], [30, 31, 32], [], [902]]
    rest = [[], [900], [901], [11], [22, 23], [33, 34, 35], [], [902]]
    table = speaker.RetokTable(list('PUEabcdB'), first, rest, device=DEV)
    rows = [[7, 3, 4, 6, 5, 2, 0, 0], [7, 3, 2, 0, 0, 0, 0, 0], [7, 6, 2, 0, 0, 0, 0, 0]]          # 8, 3 and 2 tokens
    full = [0, 10, 22, 23, 33, 34, 35, 2]
    for max_len in (5, 6, 7, 8, 9, 12):          # inside the last word's ids (5, 6), at </s> (7: lost), one past it (8), room to spare
        ids, mask, lens = _run(table, rows, case, 8, 8, max_len, 12, 1)
        _check((ids, mask, lens), _expected(table, rows, case, max_len, 12, 1), max_len)
        assert ids[0, :min(max_len, 8)].tolist() == full[:max_len] and lens.tolist() == [min(max_len, 8), 3, 2]
        assert bool((ids[0, lens[0]:] == 1).all()) and not bool(mask[0, lens[0]:].any()) and bool(mask[0, :lens[0]].all())
    assert _run(table, rows, case, 8, 8, 7, 12, 1)[0][0, 6].item() == 35          # the </s> of the 8-token row is gone at max_len 7


def _state(words, ended, end_step, pos, n_live):
    from vln_goat_amd import hipops
    st = hipops.DecodeState(words.shape[0], words.shape[1], DEV)
    st.words.copy_(words)
    st.ended.copy_(torch.tensor(ended, dtype=torch.uint8))
    st.end_step.copy_(torch.tensor(end_step, dtype=torch.int32))
    st.pos.fill_(pos)
    st.n_live.fill_(n_live)
    return st


def test_retok_rows_derives_the_width_from_the_decode_state():
    from vln_goat_amd import hipops
    case = [c for c in _golden() if c['name'] == 'rich'][0]
    table = _bpe_table(case)
    bos, eos, pad = case['bos'], case['eos'], case['pad']
    Lmax = 13

    def go(rows, ended, end_step, pos, n_live, width):
        words = torch.full((len(rows), Lmax), pad, dtype=torch.int64)
        for i, r in enumerate(rows):
            words[i, :len(r)] = torch.tensor(r)
        st = _state(words, ended, end_step, pos, n_live)
        ids = torch.full((len(rows), 32), 777, dtype=torch.int64, device=DEV)
        masks = torch.ones(len(rows), 32, dtype=torch.bool, device=DEV)
        lens = hipops.retok_rows(st.words, table, ids, masks, bos, eos, pad, AGENT_BOS, AGENT_EOS, state=st)
        want = _expected(table, [list(map(int, w[:width])) for w in words], case, 32, 32, 0)
        _check((ids.cpu(), masks.cpu(), lens.cpu()), want, width)
        return ids.cpu(), lens.cpu()
    # all rows ended: the width is max(end_step) + 2, whatever pos says
    rows = [[bos, 3, 4, 5, eos], [bos, 6, 7, 8, 9, 10, 3, 4, eos], [bos, 5, 5, 6, eos]]
    go(rows, [1, 1, 1], [3, 7, 3], 11, 0, 9)
    # two rows live at pos = Lmax - 1: every column counts; the live rows have no <EOS> and lose their last word
    live = [bos] + [3 + (i % 9) for i in range(Lmax - 1)]
    go([rows[0], live, live[::-1]], [1, 0, 0], [3, -1, -1], Lmax - 1, 2, Lmax)
    # a live row decides: pos + 1 columns, whatever the end steps say
    go(rows, [1, 0, 1], [3, -1, 3], 4, 1, 5)
    # the end step of a row that is not marked ended does not count
    go(rows, [1, 0, 1], [3, 9, 3], 11, 0, 5)
    # more rows than the block has threads: the last row's end step is the maximum
    many = [[bos, 3 + (i % 9), eos] for i in range(300)]
    many[299] = [bos, 3, 4, 5, 6, 7, eos]
    go(many, [1] * 300, [1] * 299 + [5], 12, 0, 7)
    # all ended at step 0: two columns, [<BOS>, <EOS>] -> the sentence '<BOS>'
    ids, lens = go([[bos, eos]] * 3, [1, 1, 1], [0, 0, 0], 1, 0, 2)
    assert ids[0, :lens[0]].tolist() == [AGENT_BOS] + table.first[bos] + [AGENT_EOS]


def test_retok_rows_status_words():
    from vln_goat_amd import hipops
    case = [c for c in _golden() if c['name'] == 'small'][0]
    V = len(case['vocab'])
    table = _synthetic_table(V)
    good = [7, 3, 4, 2, 0, 0]
    with pytest.raises(ValueError, match='row 1.*vocabulary'):
        _run(table, [good, [7, 3, V, 2, 0, 0], good], case, 6, 6, 16, 16, 1)
    with pytest.raises(ValueError, match='row 0.*fewer than 2 columns'):
        _run(table, [good, good], case, 1, 6, 16, 16, 1)
    with pytest.raises(ValueError, match='fewer than 2 columns'):          # ... or more columns than the tensor has
        _run(table, [good], case, 7, 6, 16, 16, 1)
    with pytest.raises(ValueError, match='row 2.*one run'):
        _run(table, [good, good, [3, 3, 3, 3, 3, 3]], case, 6, 6, 16, 16, 1)
    # a word outside the vocabulary behind `width` is never read; check=False leaves the words for the caller
    status = torch.full((4,), 99, dtype=torch.int32, device=DEV)
    rows = [good, [7, 3, -1, 2, 0, 0], [7, 7, 7, 7, 7, 7], [7, 3, 4, 2, 0, V]]
    ids, mask, lens = _run(table, rows, case, 5, 6, 16, 16, 1, status=status, check=False)
    assert status.tolist() == [0, 2, 4, 0]
    want = _expected(table, [good[:5], rows[3][:5]], case, 16, 16, 1)
    _check((ids[[0, 3]], mask[[0, 3]], lens[[0, 3]]), want, 'good rows next to bad ones')
    assert lens[[1, 2]].tolist() == [0, 0] and bool((ids[[1, 2]] == 1).all()) and not bool(mask[[1, 2]].any())
    with pytest.raises(ValueError, match='row 1'):
        hipops.check_retok_status(status)
    # the golden rows the reference raises on
    for r in case['rows']:
        if r.get('raises') and len(r['row']) >= 2:
            with pytest.raises(ValueError, match='one run'):
                _run(table, [r['row']], case, len(r['row']), len(r['row']), 16, 16, 1)


# ------------------------------------------------------------------------------------------------ goat_scale_cols
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _noise(kind, D, g):
    if kind == 'zeros':
        return torch.zeros(D)
    if kind == 'keep':
        return torch.full((D,), 1.0 / (1.0 - 0.3))
    return torch.where(torch.rand(D, generator=g) < 0.5, torch.zeros(D), torch.full((D,), 2.0)) + 0.37 * (torch.arange(D) % 3 == 1)


def _scale_case(dtype, rows, D, ld, kind, g, offset=0):
    from vln_goat_amd import hipops
    buf = torch.randn(rows * ld + offset, generator=g).to(dtype).to(DEV)
    x = buf[offset:].view(rows, ld)                         # offset 1: a base that is not 16-byte aligned
    noise = _noise(kind, D, g).to(DEV)
    want = x.clone()
    want[:, :D] = (x[:, :D].float() * noise).to(dtype)
    before = x.clone()
    out = hipops.scale_cols(x, noise)
    assert out.data_ptr() != x.data_ptr() and torch.equal(_bits(x), _bits(before))          # out of place: the input is untouched
    assert torch.equal(_bits(out), _bits(want)), (dtype, rows, D, ld, kind, offset, 'out of place')
    same = hipops.scale_cols(x, noise, out=x)
    assert same is x and torch.equal(_bits(x), _bits(want)), (dtype, rows, D, ld, kind, offset, 'in place')


@pytest.mark.parametrize('D', [8, 20, 768])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_scale_cols_equals_one_float32_multiply(dtype, D):
    g = torch.Generator().manual_seed(D)
    for rows in (1, 5, 257):
        for ld in (D, D + 128, D + 3):
            for kind in ('zeros', 'keep', 'mixed'):
                _scale_case(dtype, rows, D, ld, kind, g)
    _scale_case(dtype, 5, D, D + 128, 'mixed', g, offset=1)          # chunkable ld on a misaligned base: the element path


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_scale_cols_beyond_one_grid(dtype):
    """more 16-byte chunks (ld 896) and more single elements (ld 771) than one pass of the grid covers: the strided loops"""
    g = torch.Generator().manual_seed(1)
    _scale_case(dtype, 5000, 768, 896, 'mixed', g)
    _scale_case(dtype, 1500, 768, 771, 'mixed', g)


def test_scale_cols_keeps_special_values_behind_d():
    from vln_goat_amd import hipops
    x = torch.zeros(3, 24, device=DEV)
    x[:, 8:] = torch.tensor([float('nan'), float('inf'), -0.0, 1e-42] * 4, device=DEV)
    x[:, :8] = torch.arange(24, device=DEV, dtype=torch.float32).view(3, 8)
    noise = torch.tensor([0.0, 2.0] * 4, device=DEV)
    out = hipops.scale_cols(x, noise)
    assert torch.equal(_bits(out[:, 8:].contiguous()), _bits(x[:, 8:].contiguous()))
    assert torch.equal(out[:, :8], x[:, :8] * noise)


# ------------------------------------------------------------------------------------------------ VLNBert('panorama') with env_noise
def _flat(out):
    return [t for t in (out if isinstance(out, (tuple, list)) else [out]) if torch.is_tensor(t)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_vlnbert_panorama_with_env_noise(dtype):
    import collections
    import vln_goat_amd
    from vln_goat_amd import hipops, nav_model, synth
    args = SimpleNamespace(num_l_layers=1, num_x_layers=1, num_pano_layers=1, dropout=0.5, feat_dropout=0.5, do_back_img=True, do_back_txt=True,
                           do_front_img=True, do_front_his=True, do_front_txt=True, vocab_size=500, mode='train', do_back_txt_type='type_2',
                           do_back_img_type='type_1', do_add_method='door', bert_ckpt_file=None)
    vln_goat_amd.set_compute_dtype(dtype)
    rng = (hipops.RngState.base, hipops.RngState.seed, hipops.RngState.counter)
    try:
        torch.manual_seed(0)
        net = nav_model.VLNBert(args)
        net.vln_bert.load_state_dict(synth.seeded_state_dict(net.vln_bert, seed=11))
        net = net.cuda().train()
        ep = synth.make_nav_episode(B=2, L=30, n_steps=2, seed=1, vocab_size=500)
        st = ep['steps'][0]
        pin = {k: st[k].cuda() for k in ('view_img_fts', 'loc_fts', 'nav_types', 'view_lens')}
        pin.update(z_img_features=ep['z_img_features'].cuda(), z_img_pzs=ep['z_img_pzs'].cuda())
        x = pin['view_img_fts']
        with torch.no_grad():
            noise = hipops.dropout(torch.ones(x.shape[-1], device=DEV), 0.5)
            assert 0.3 < float((noise == 0).float().mean()) < 0.7 and set(noise.unique().tolist()) == {0.0, 2.0}

            def call(batch, model=net):
                hipops.manual_seed(5)
                return _flat(model('panorama', batch))
            with_key = call(dict(pin, env_noise=noise))
            by_torch = call(dict(pin, view_img_fts=(x.to(dtype).float() * noise).to(dtype), already_dropout=True))
            assert len(with_key) == len(by_torch) >= 2
            for a, b in zip(with_key, by_torch):
                assert torch.equal(a, b)
            assert torch.equal(x, ep['steps'][0]['view_img_fts'].cuda())          # the caller's features are not scaled in place
            # without the key: the per-element drop_env of before, the same launches in the same order
            plain = call(dict(pin))
            assert not torch.equal(plain[0], with_key[0])
            hipops.manual_seed(5)
            dropped = hipops.dropout(x.to(dtype).contiguous(), 0.5)
            parent = _flat(net.vln_bert('panorama', collections.defaultdict(lambda: None, dict(pin, view_img_fts=dropped))))
            for a, b in zip(plain, parent):
                assert torch.equal(a, b)
            # eval mode: ones in, nothing changes
            net.eval()
            ones = torch.ones_like(noise)
            for a, b in zip(call(dict(pin, env_noise=ones)), call(dict(pin))):
                assert torch.equal(a, b)
    finally:
        vln_goat_amd.set_compute_dtype(torch.float32)
        hipops.RngState.base, hipops.RngState.seed, hipops.RngState.counter = rng


# ------------------------------------------------------------------------------------------------ BackTranslator
def _small_speaker(F, image_feat_size, V, seed=4):
    from vln_goat_amd import speaker
    cfg = speaker.default_config(h_dim=128, wemb=64, proj_hidden=128, speaker_layer_num=1, speaker_head_num=2, speaker_dropout=0.2,
                                 featdropout=0.3, image_feat_size=image_feat_size, attn_dropout_always=False)
    torch.manual_seed(seed)
    return speaker.Transpeaker(F, 128, 64, V, cfg).cuda().eval()


def _pipeline(table, words, case, L, fill=0):
    return _expected(table, [list(map(int, w)) for w in words.cpu()], case, L, L, fill)


def test_backtranslator_run_end_to_end():
    from vln_goat_amd import speaker
    case = [c for c in _golden() if c['name'] == 'rich'][0]
    table = _bpe_table(case)
    V, B, T, F, D, L, md = len(case['vocab']), 3, 4, 64, 48, 32, 12
    model = _small_speaker(F, D, V)
    kw = dict(bos=case['bos'], eos=case['eos'], pad=case['pad'], unk=case['unk'])
    g = torch.Generator().manual_seed(9)
    can, img = torch.randn(B, T, F, generator=g).cuda(), torch.randn(B, T, 36, F, generator=g).cuda()
    bt = speaker.BackTranslator(model, table, B, md, T, agent_bos=AGENT_BOS, agent_eos=AGENT_EOS, **kw)
    out_ids = torch.full((B, L), 777, dtype=torch.int64, device=DEV)
    out_masks = torch.ones(B, L, dtype=torch.bool, device=DEV)
    lens = bt.run(can, img, out_ids, out_masks)
    words = speaker.infer_batch_cached(model, can, img, max_decode=md, **kw)
    want = _pipeline(table, words, case, L)
    _check((out_ids.cpu(), out_masks.cpu(), lens.cpu()), want, 'no noise')
    assert bt.instr_encodings() == [want[0][i, :want[2][i]].tolist() for i in range(B)]
    assert all(2 <= n <= L for n in want[2].tolist())
    # the shared mask: image columns of both inputs times noise, the encoder's own feature dropout skipped
    noise = torch.where(torch.rand(D, generator=g) < 0.5, torch.zeros(D), torch.full((D,), 2.0)).cuda()
    assert bt.noise.shape == (D,) and bt.noise.dtype == torch.float32
    bt.noise.copy_(noise)
    lens = bt.run(can, img, out_ids, out_masks, noise=bt.noise)
    scale = torch.cat([noise, torch.ones(F - D, device=DEV)])
    words_n = speaker.infer_batch_cached(model, can * scale, img * scale, max_decode=md, already_dropfeat=True, **kw)
    _check((out_ids.cpu(), out_masks.cpu(), lens.cpu()), _pipeline(table, words_n, case, L), 'noise')
    # draw_noise: all ones in eval mode, zeros and 1 / (1 - p) in train mode
    env = SimpleNamespace(drop_env=torch.nn.Dropout(0.5).eval())
    assert torch.equal(bt.draw_noise(env), torch.ones(D, device=DEV))
    env.drop_env.train()
    assert set(bt.draw_noise(env).unique().tolist()) == {0.0, 2.0}


def test_device_walk_on_a_device_written_instruction():
    from test_device_navigator_gpu import _model, _two_scans
    from vln_goat_amd import features, rollout, speaker, synth
    B, T = 2, 3
    case = [c for c in _golden() if c['name'] == 'rich'][0]
    table = _bpe_table(case)
    scans, eps = _two_scans(24, 3, 29, 2, B, T, seed=21)
    rs = np.random.RandomState(2)
    arrays = {'%s_%s' % (sc.name, vp): rs.standard_normal((36, 768)).astype(np.float32) for sc in scans for vp in sc.vpids}
    store = features.FeatureStore.from_arrays(arrays, dtype=torch.float32).to('cuda')
    sim = rollout.GraphSim(store)
    model = _model()
    _, _, _, dicts = synth.make_rollout_case()
    ex = synth.rollout_extras(dicts, B, 'cuda')
    te = rollout.TeacherEpisode(sim, store, n_steps=T, text_len=32, pano_width=40)
    bufs = rollout.EpisodeBuffers(te.plan(eps))
    walk = rollout.ArgmaxEpisode(te, lambda mode, batch: model(mode, batch), bufs, ex)
    tables = rollout.ScanTables(scans, store)
    nav = rollout.DeviceNavigator(te, tables, bufs, 'argmax')
    # the speaker over the ground-truth paths
    img, can, _ = speaker.path_features(sim, store, eps, angle_size=128)
    spk = _small_speaker(768 + 128, 768, len(case['vocab']))
    bt = speaker.BackTranslator(spk, table, B, 12, img.shape[1], case['bos'], case['eos'], case['pad'], case['unk'], AGENT_BOS, AGENT_EOS)
    bt.run(can, img, bufs.t['txt_ids'], bufs.t['txt_masks'])
    traj_d, actions_d, _, _ = nav.walk(walk, eps, act=lambda t: walk.back, text='device')
    ids_d, masks_d = bufs.t['txt_ids'].clone(), bufs.t['txt_masks'].clone()
    enc = bt.instr_encodings()
    assert all(2 <= len(e) <= 32 for e in enc) and [len(e) for e in enc] == masks_d.sum(1).tolist()
    assert any(e != list(eps[i]['instr_encoding']) for i, e in enumerate(enc))          # not the instruction the episodes came with
    bufs.t['txt_ids'].zero_()
    host_eps = [dict(e, instr_encoding=enc[i]) for i, e in enumerate(eps)]
    traj_h, actions_h, _, _ = nav.walk(walk, host_eps, act=lambda t: walk.back, text='host')
    assert torch.equal(bufs.t['txt_ids'], ids_d) and torch.equal(bufs.t['txt_masks'], masks_d)
    assert len(actions_d) == len(actions_h) and all(np.array_equal(a, b) for a, b in zip(actions_d, actions_h))
    assert [t['path'] for t in traj_d] == [t['path'] for t in traj_h]
    with pytest.raises(ValueError, match='text'):
        nav.begin(eps, text='gpu')
