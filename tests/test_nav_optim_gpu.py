"""The fine-tuning update on the device: optim.FusedTorchOptim (goat_grad_sqnorm + goat_optim_step + goat_optim_advance) against what the
reference's iteration calls — torch.optim.<X>(params, lr) with torch's defaults behind clip_grad_norm_(params, 40.) — run at test time on
float32 CPU copies.  Bounds: those of the pre-training optimizer's trace test (test_train_step_gpu.py)."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

TORCH = {'adamW': torch.optim.AdamW, 'adam': torch.optim.Adam, 'rms': torch.optim.RMSprop, 'sgd': torch.optim.SGD}
MOMENTS = {'adamW': ('exp_avg', 'exp_avg_sq'), 'adam': ('exp_avg', 'exp_avg_sq'), 'rms': ('square_avg',), 'sgd': ()}
M_TOL = {'exp_avg': (1e-6, 1e-3), 'exp_avg_sq': (3e-6, 1e-6), 'square_avg': (3e-6, 1e-6)}         # (relative, floor of the scale)

# where the kernel can go wrong: tiny tensors, a bias, exactly one chunk, a one-element second chunk, a matrix across a chunk boundary, an odd
# tail, a K-padded 7-wide Linear, fused QKV with biases; `shifted` is a view 4 bytes off the 16-byte grid (the scalar path on > 1 wavefront)
SHAPES = [('s1', (1,)), ('s3', (3,)), ('bias', (768,)), ('chunk', (65536,)), ('chunk1', (65537,)), ('mat', (96, 768)), ('odd', (100003,)),
          ('w7', (768, 7)), ('q', (64, 64)), ('k', (64, 64)), ('v', (64, 64)), ('bq', (64,)), ('bk', (64,)), ('bv', (64,)), ('shifted', (1029,)),
          ('frozen', (16,)), ('unused', (8,))]
SMALL = [n for n, _ in SHAPES if n not in ('chunk', 'odd', 'mat')]
UNCOVERED = ('frozen', 'unused')


def _case(names=None, copies=True, seed=0, tasks=('nav',), tasks_of=None):
    """parameters on the device, the hand-made arena (every tensor but `unused` used by `tasks`, or by tasks_of[name]), and the cached
    operand copies the forward passes would have made"""
    from vln_goat_amd import dp, hipops
    gen = torch.Generator().manual_seed(seed)
    params, base = {}, None
    for n, shp in SHAPES:
        if names is not None and n not in names:
            continue
        w = torch.randn(shp, generator=gen) * 0.5
        if n == 'shifted':
            base = torch.zeros(shp[0] + 1, device='cuda')
            base[1:].copy_(w)
            params[n] = torch.nn.Parameter(base[1:])
            assert params[n].data_ptr() % 16 == 4
        else:
            params[n] = torch.nn.Parameter(w.cuda(), requires_grad=n != 'frozen')
    usage = {id(p): (set() if n == 'unused' else set((tasks_of or {}).get(n, tasks))) for n, p in params.items()}
    arena = dp.GradArena(list(params.values()), usage).attach()
    assert all(id(params[n]) not in arena.views for n in UNCOVERED if n in params)
    bf = torch.bfloat16
    if copies:
        with torch.no_grad():
            hipops.linear(torch.randn(4, 7, device='cuda').to(bf), params['w7'], None)                                  # K-padded bf16 copy [768, 8]
            hipops.multi_linear(torch.randn(4, 64, device='cuda').to(bf), tuple(params[n] for n in 'qkv'), tuple(params[n] for n in ('bq', 'bk', 'bv')))
        for n in ('s3', 'bias', 'chunk1', 'mat', 'odd', 'shifted', 'q'):
            if n in params:
                hipops._shadow(params[n], bf)
        hipops._shadow(params['bias'], torch.float32)               # a float32 image: not one of the kernel's slots, rebuilt by refresh_shadows
    return params, arena


def _grads(params, seed, scale):
    """Seeded normal gradients of standard deviation `scale`, rounded to a power-of-two grid q of 5-6 steps per sigma.  Every square is then
    a multiple of q^2 and every partial sum of squares below 2^24 q^2: float32 adds them exactly in ANY order, so the oracle and the device
    see the same squared norm whatever the order of torch's vector lanes or of the kernel's atomic sum.  (torch's float32 norm of 3e5
    free-form values is itself 5e-7 off their float64 norm; through the clip coefficient that alone moves the first moment of the
    one-element tensor by more than its bound of 1e-9.)"""
    q = 2.0 ** math.floor(math.log2(scale / 4))
    gen = torch.Generator().manual_seed(seed)
    g = {n: torch.round(torch.randn(p.shape, generator=gen) * (scale / q)) * q for n, p in params.items() if n not in UNCOVERED}
    assert sum(float(x.double().pow(2).sum()) for x in g.values()) < 2 ** 24 * q * q
    return g


def _oracle(params, algo, lr):
    cpu = {n: torch.nn.Parameter(p.detach().cpu().clone(), requires_grad=p.requires_grad) for n, p in params.items()}
    return cpu, TORCH[algo](list(cpu.values()), lr=lr)


def _oracle_step(cpu, topt, grads, max_norm=40.0):
    for n, p in cpu.items():
        p.grad = grads[n].clone() if n in grads else None
    norm = torch.nn.utils.clip_grad_norm_(list(cpu.values()), max_norm)
    topt.step()
    return float(norm)


def _load(arena, params, grads):
    for n, g in grads.items():
        arena.views[id(params[n])].copy_(g)


def _close(got, ref, rel, floor, what):
    err, scale = float((got - ref).abs().max()), max(floor, float(ref.abs().max()))
    assert err <= rel * scale, (what, err, scale)


def _check_params(params, cpu, what):
    for n, p in params.items():
        got, ref = p.detach().cpu(), cpu[n].detach()
        err = float((got - ref).abs().max())
        assert err <= 2e-6 * max(1.0, float(ref.abs().max())) + 1e-9, (what, n, err)


def _check_moments(opt, topt, params, cpu, algo, what):
    for n, p in params.items():
        if n in UNCOVERED:
            continue
        st, ref = opt.state_of(p), topt.state[cpu[n]]
        for k in MOMENTS[algo]:
            _close(st[k].detach().cpu(), ref[k], *M_TOL[k], (what, n, k))


def _check_copies(params):
    """every cached copy equals the rounded float32 master (-> number of copies seen, by kind)"""
    from vln_goat_amd import shadows
    by_id = {id(p): p for p in params.values()}
    seen = {}
    for n, p in params.items():
        for key, (_, t) in (p.__dict__.get('_goat_shadow') or {}).items():
            kind = shadows.key_kind(key)
            if kind == shadows.CAT:
                want = torch.cat([by_id[i].detach() for i in shadows.member_ids(key)], 0).to(key[1])
            elif kind == shadows.CATB:
                want = torch.cat([by_id[i].detach().float() for i in shadows.member_ids(key)], 0)
            elif kind == shadows.PLAIN:
                want = shadows._build_shadow(p, key)
                if key[2]:
                    kind = 'kpad'
                    assert not bool(t[:, p.shape[1]:].any()), n
                elif key[0] == torch.float32:
                    kind = 'f32'
            else:
                want = shadows._BUILD[kind](p, key)
            assert torch.equal(t, want), (n, key)
            seen[kind] = seen.get(kind, 0) + 1
    return seen


@pytest.mark.parametrize('algo', ['adamW', 'adam', 'rms', 'sgd'])
def test_three_steps_match_torch(algo):
    """Three steps of every algorithm on the hand-made arena: step 0 is clipped (norm > 40), steps 1-2 are not, the learning rate changes before
    step 2.  After every step: parameters, moments, gradient norm within the bounds; every cached operand copy equals the rounded master and is
    still the cached object; the tensors outside the arena keep their bits; the device counter equals the step."""
    from vln_goat_amd import hipops, optim
    params, arena = _case()
    start = {n: params[n].detach().clone() for n in UNCOVERED}
    cached = {n: hipops._shadow(params[n], torch.bfloat16) for n in ('mat', 'chunk1', 'shifted')}
    cpu, topt = _oracle(params, algo, 1e-3)
    opt = optim.FusedTorchOptim(params.items(), arena, algo=algo, lr=1e-3)
    assert len(opt.params) == len(SHAPES) - 2 and opt.steps_done() == 0
    for step, (scale, lr) in enumerate(((0.1, 1e-3), (0.05, 1e-3), (0.04, 4e-4))):
        grads = _grads(params, 100 + step, scale)
        opt.param_groups[0]['lr'] = topt.param_groups[0]['lr'] = lr
        ref_norm = _oracle_step(cpu, topt, grads)
        assert (ref_norm > 40.0) == (step == 0), (step, ref_norm)
        _load(arena, params, grads)
        opt.step(max_norm=40.0)
        torch.cuda.synchronize()
        norm = opt.last_grad_norm()
        print('%s step %d: norm %.6f (torch %.6f)' % (algo, step, norm, ref_norm))
        assert abs(norm - ref_norm) <= 1e-4 * ref_norm, (step, norm, ref_norm)
        _check_params(params, cpu, (algo, step))
        _check_moments(opt, topt, params, cpu, algo, (algo, step))
        seen = _check_copies(params)
        assert seen == {'plain': 7, 'kpad': 1, 'cat': 1, 'catb': 1, 'f32': 1}, seen
        assert opt.last_refreshed == 1                                   # the float32 image only: every bf16 copy was the kernel's
        for n, t in cached.items():
            assert hipops._shadow(params[n], torch.bfloat16) is t, n
        for n in UNCOVERED:
            assert torch.equal(params[n].detach(), start[n]), n
        assert opt.steps_done() == step + 1 and opt.state_of(params['mat'])['step'] == step + 1


@pytest.mark.parametrize('clipped', [False, True])
def test_captured_step_equals_eager_steps(clipped):
    """step() captured once in hipops.graph, replayed three times with new gradients in the arena and set_lr between the replays, against
    three eager steps of a twin: bit for bit when no step clips (the coefficient is exactly 1 whatever the order of the norm's atomic sum),
    within the bounds when one does."""
    from vln_goat_amd import hipops, optim
    runs = []
    for captured in (True, False):
        params, arena = _case(names=SMALL + ['mat'])
        opt = optim.FusedTorchOptim(params.items(), arena, algo='adamW', lr=1e-3)
        if captured:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with hipops.graph(g):
                opt.step(max_norm=40.0)
            torch.cuda.synchronize()
            assert opt.steps_done() == 0                                  # a capture runs nothing
        norms = []
        for i, (scale, lr) in enumerate(((0.05, 1e-3), (2.0 if clipped else 0.06, 7e-4), (0.03, 2e-4))):
            _load(arena, params, _grads(params, 200 + i, scale))
            opt.set_lr(lr)
            if captured:
                g.replay()
            else:
                opt.step(max_norm=40.0)
            norms.append(opt.last_grad_norm())
        torch.cuda.synchronize()
        assert opt.steps_done() == 3
        runs.append((params, opt, norms))
    (pa, oa, na), (pb, ob, nb) = runs
    print('captured norms %s, eager norms %s' % (na, nb))
    assert [x > 40.0 for x in nb] == [False, clipped, False], nb
    _check_copies(pa)
    for n in pa:
        if clipped:
            _close(pa[n].detach(), pb[n].detach(), 2e-6, 1.0, n)
        else:
            assert torch.equal(pa[n].detach(), pb[n].detach()), n
        if n in UNCOVERED:
            continue
        sa, sb = oa.state_of(pa[n]), ob.state_of(pb[n])
        for k in MOMENTS['adamW']:
            if clipped:
                _close(sa[k], sb[k], *M_TOL[k], (n, k))
            else:
                assert torch.equal(sa[k], sb[k]), (n, k)
    for x, y in zip(na, nb):
        assert abs(x - y) <= 1e-4 * y


@pytest.mark.parametrize('algo', ['adamW', 'rms'])
def test_state_interchanges_with_torch_on_the_device(algo):
    """Two fused steps -> state_dict() -> torch's optimizer on CPU clones -> a third step on both agrees; and two torch steps -> load_state_dict
    into a fresh fused optimizer -> a third step agrees."""
    from vln_goat_amd import optim
    names = SMALL + ['mat']
    # fused -> torch
    params, arena = _case(names=names, copies=False)
    opt = optim.FusedTorchOptim(params.items(), arena, algo=algo, lr=1e-3)
    for i in range(2):
        _load(arena, params, _grads(params, 300 + i, 0.05))
        opt.step(max_norm=40.0)
    sd = opt.state_dict()
    assert sorted(sd['state']) == [i for i, n in enumerate(params) if n not in UNCOVERED]
    assert all(float(e['step']) == 2.0 and all(e[k].is_cuda for k in MOMENTS[algo]) for e in sd['state'].values())
    cpu, topt = _oracle(params, algo, 0.5)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['lr'] == 1e-3
    grads = _grads(params, 302, 0.05)
    _oracle_step(cpu, topt, grads)
    _load(arena, params, grads)
    opt.step(max_norm=40.0)
    torch.cuda.synchronize()
    _check_params(params, cpu, (algo, 'fused->torch'))
    _check_moments(opt, topt, params, cpu, algo, (algo, 'fused->torch'))
    # torch -> fused
    params, arena = _case(names=names, copies=False, seed=1)
    cpu, topt = _oracle(params, algo, 1e-3)
    for i in range(2):
        _oracle_step(cpu, topt, _grads(params, 310 + i, 0.05))
    with torch.no_grad():
        for n, p in params.items():
            p.copy_(cpu[n])
    opt = optim.FusedTorchOptim(params.items(), arena, algo=algo, lr=0.5)
    opt.load_state_dict(topt.state_dict())
    assert opt.steps_done() == 2 and opt.param_groups[0]['lr'] == 1e-3
    grads = _grads(params, 312, 0.05)
    _oracle_step(cpu, topt, grads)
    _load(arena, params, grads)
    opt.step(max_norm=40.0)
    torch.cuda.synchronize()
    assert opt.steps_done() == 3
    _check_params(params, cpu, (algo, 'torch->fused'))
    _check_moments(opt, topt, params, cpu, algo, (algo, 'torch->fused'))


def test_fused_adamw_three_steps_on_the_edge_shapes():
    """The pre-training update (optim.FusedAdamW: goat_grad_sqnorm + goat_adamw_step) on the shapes above, which its own trace test
    (test_train_step_gpu.py, largest tensor 300x64, everything aligned and below one chunk) never reaches: chunk boundaries, the odd tail, the
    shifted view, the K-padded and the concatenated copies.  Two task keys; `s3` belongs to 'a' only, so its step count and bias correction
    lag.  Step 0 is clipped (norm > 5), steps 1-2 are not, the learning rate changes before step 2; `bias` is in the no-decay group.
    Against helpers.clip_adamw_step (pinned bit for bit to the reference's trace by test_adamw_restatement.py), bounds of the trace test."""
    from helpers import clip_adamw_step
    from vln_goat_amd import optim
    params, arena = _case(tasks=('a', 'b'), tasks_of={'s3': ('a',)})
    start = {n: params[n].detach().clone() for n in UNCOVERED}
    cpu = {n: p.detach().cpu().clone() for n, p in params.items() if n not in UNCOVERED}
    wd = {n: 0.0 if any(nd in n for nd in optim.NO_DECAY) else 0.01 for n in cpu}
    state = {}
    opt = optim.FusedAdamW(params.items(), arena, lr=1e-3, betas=(0.9, 0.98), weight_decay=0.01)
    assert opt.param_groups[1]['names'] == ['bias'] and len(opt.param_groups[0]['names']) == len(SHAPES) - 3
    for step, (task, scale, lr) in enumerate((('a', 0.1, 1e-3), ('b', 0.00625, 1e-3), ('a', 0.005, 4e-4))):
        grads = _grads(params, 400 + step, scale)
        if task == 'b':
            del grads['s3']
        ref_norm = clip_adamw_step(cpu, grads, state, lr, wd, betas=(0.9, 0.98), eps=1e-6, max_norm=5.0)
        assert (ref_norm > 5.0) == (step == 0), (step, ref_norm)
        arena.bind(task)
        arena.flat.zero_()
        _load(arena, params, grads)
        for g in opt.param_groups:
            g['lr'] = lr
        opt.step(task, max_norm=5.0)
        torch.cuda.synchronize()
        norm = opt.last_grad_norm()
        print('adamw step %d (%s): norm %.6f (restatement %.6f)' % (step, task, norm, ref_norm))
        assert abs(norm - ref_norm) <= 1e-4 * ref_norm, (step, norm, ref_norm)
        for n, ref in cpu.items():
            err = float((params[n].detach().cpu() - ref).abs().max())
            print('  %-8s |p - ref| %.3e' % (n, err))
            assert err <= 2e-6 * max(1.0, float(ref.abs().max())) + 1e-9, (step, n, err)
            st = opt.state_of(params[n])
            if n in state:
                for k in MOMENTS['adamW']:
                    _close(st[k].detach().cpu(), state[n][k], *M_TOL[k], (step, n, k))
        _check_copies(params)
        for n in UNCOVERED:
            assert torch.equal(params[n].detach(), start[n]), n
    assert opt.steps[id(params['s3'])] == 2 == state['s3']['step'] and all(opt.steps[id(params[n])] == 3 for n in cpu if n != 's3')


def _to_device(ep):
    mv = lambda x: x.cuda() if torch.is_tensor(x) else x
    return {k: ([{kk: mv(vv) for kk, vv in st.items()} for st in v] if k == 'steps' else mv(v)) for k, v in ep.items()}


def test_on_the_model_matches_torch_adamw():
    """A 1/1/1-layer VLNBert (fp32 path, dropout off), three iterations of a two-step episode: FusedTorchOptim('adamW', lr=1e-4) next to the
    same model under torch.optim.AdamW(lr=1e-4) + clip_grad_norm_(40.).  Per parameter ||d_fused - d_torch|| <= 2e-2 ||d_torch|| + 1e-9 (parameters
    whose gradient is rounding noise are normalised to +-lr by any Adam and are left out, as in
    test_fused_adamw_on_the_model_matches_torch_adamw); parameters without a gradient keep their bits."""
    from vln_goat_amd import dp, nav_model, optim, synth
    args = SimpleNamespace(num_l_layers=1, num_x_layers=1, num_pano_layers=1, dropout=0.0, feat_dropout=0.0, do_back_img=True, do_back_txt=True,
                           do_front_img=True, do_front_his=True, do_front_txt=True, vocab_size=500, mode='train', do_back_txt_type='type_2',
                           do_back_img_type='type_1', do_add_method='door', bert_ckpt_file=None)
    ep = _to_device(synth.make_nav_episode(B=2, L=20, n_steps=2, seed=1, vocab_size=500))
    finals = []
    for fused in (False, True):
        torch.manual_seed(0)
        net = nav_model.VLNBert(args).cuda().eval()

        def episode():
            loss, _ = synth.run_nav_episode(lambda m, b: net(m, dict(b)), ep, device='cuda')
            loss.backward()
        episode()
        wrapper = dp.GoatDataParallel(net)
        wrapper.record_usage('nav')
        for p in net.parameters():
            p.grad = None
        arena = wrapper.build_arena()
        if fused:
            opt = optim.FusedTorchOptim(net.named_parameters(), arena, algo='adamW', lr=1e-4)
        else:
            opt = torch.optim.AdamW(list(net.parameters()), lr=1e-4)
        start = {n: p.detach().clone() for n, p in net.named_parameters()}
        noisy, norms = set(), []
        for it in range(3):
            arena.zero('nav')
            episode()
            if fused:
                opt.step(max_norm=40.0)
                norms.append(opt.last_grad_norm())
            else:
                gmax = max(float(p.grad.norm()) for p in net.parameters() if p.grad is not None)
                noisy |= {n for n, p in net.named_parameters() if p.grad is not None and float(p.grad.norm()) < 1e-5 * gmax}
                norms.append(float(torch.nn.utils.clip_grad_norm_(list(net.parameters()), 40.)))
                opt.step()
        torch.cuda.synchronize()
        finals.append(({n: p.detach().clone() for n, p in net.named_parameters()}, start, noisy, norms, {n for n, p in net.named_parameters() if id(p) in arena.views}))
    (a, start, noisy, na, in_arena), (b, _, _, nb, _) = finals
    print('torch norms %s, fused norms %s, %d noisy' % (na, nb, len(noisy)))
    assert all(abs(x - y) <= 1e-3 * x for x, y in zip(na, nb)), (na, nb)
    moved, still = 0, 0
    for n in a:
        if n not in in_arena:
            assert torch.equal(b[n], start[n]) and torch.equal(a[n], start[n]), n       # no gradient: bit-identical to the start
            still += 1
            continue
        if n in noisy or 'key.bias' in n or 'in_proj_bias' in n:        # (key biases: softmax is shift-invariant, their gradient is rounding noise)
            continue
        da, db = (a[n] - start[n]).double(), (b[n] - start[n]).double()
        moved += 1
        assert float((db - da).norm()) <= 2e-2 * float(da.norm()) + 1e-9, (n, float((db - da).norm()), float(da.norm()))
    print('%d parameters moved, %d without a gradient' % (moved, still))
    assert moved > 100 and still > 0


def test_bf16_copies_stay_coherent_under_a_captured_episode():
    """bf16 path: after two fused steps every cached bf16 copy equals the rounded master, and a TeacherEpisode graph captured BEFORE the steps,
    replayed after them, returns the loss of a fresh eager pass with every cache dropped (copies rebuilt from the masters) — compared as
    test_fused_adamw_keeps_the_bf16_shadows_coherent compares its forward passes: equal."""
    import vln_goat_amd
    from vln_goat_amd import dp, features, hipops, nav_model, optim, rollout, synth
    ep_args = dict(num_l_layers=2, num_x_layers=2, num_pano_layers=2, dropout=0.5, feat_dropout=0.4, do_back_img=True, do_back_txt=True,
                   do_front_img=True, do_front_his=True, do_front_txt=True, vocab_size=1200, mode='train', do_back_txt_type='type_2',
                   do_back_img_type='type_1', do_add_method='door')
    scan, feats, eps, dicts = synth.make_rollout_case()
    torch.manual_seed(0)
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(SimpleNamespace(**ep_args)))
    model.load_state_dict(synth.seeded_state_dict(model, seed=11))
    model = model.cuda().eval()
    store = features.FeatureStore.from_arrays({'%s_%s' % (scan.name, vp): feats[i] for i, vp in enumerate(scan.vpids)}, dtype=torch.bfloat16).to('cuda')
    sim = rollout.GraphSim(store)
    vln_goat_amd.set_compute_dtype(torch.bfloat16)
    try:
        ex = synth.rollout_extras(dicts, 3, 'cuda')
        te = rollout.TeacherEpisode(sim, store, n_steps=4, text_len=32, pano_width=40)
        bufs = rollout.EpisodeBuffers(te.plan(eps))
        call = lambda mode, batch: model(mode, batch)
        te.body(call, bufs, ex).backward()
        wrapper = dp.GoatDataParallel(model)
        wrapper.record_usage('nav')
        for p in model.parameters():
            p.grad = None
        arena = wrapper.build_arena()
        out = {}

        def step():
            arena.zero('nav')
            loss = te.body(call, bufs, ex)
            loss.backward()
            out['loss'] = loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        out.clear()          # (no warm-up autograd graph alive during the capture)
        g = torch.cuda.CUDAGraph()
        with hipops.graph(g):
            step()
        opt = optim.FusedTorchOptim(model.named_parameters(), arena, algo='adamW', lr=1e-3)      # a large step: stale copies would show far above the bf16 noise
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        for _ in range(2):
            g.replay()
            opt.step(max_norm=40.0)
        torch.cuda.synchronize()
        assert opt.steps_done() == 2
        assert sum(1 for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])) > 100
        seen = _check_copies(dict(model.named_parameters()))
        print('copies checked: %s, rebuilt by torch ops after the kernel: %d' % (seen, opt.last_refreshed))
        assert seen.get('plain', 0) > 10 and seen.get('cat', 0) >= 1, seen
        g.replay()
        torch.cuda.synchronize()
        got = out['loss'].detach().float().clone()
        for p in model.parameters():
            p.__dict__.pop('_goat_shadow', None)
        fresh = te.body(call, bufs, ex).detach().float()
        torch.cuda.synchronize()
        print('replayed loss %.8f, fresh eager loss %.8f' % (float(got), float(fresh)))
        assert torch.equal(got, fresh), (float(got), float(fresh))
    finally:
        vln_goat_amd.set_compute_dtype(torch.float32)
