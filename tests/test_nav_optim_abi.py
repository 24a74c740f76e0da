"""The fine-tuning update without a GPU: goat_optim_step / goat_optim_advance are exported, bound and validate their arguments before
any launch, and optim.FusedTorchOptim on a CPU arena speaks torch's optimizer checkpoint format in both directions (no launch)."""
import ctypes

import pytest
import torch


def _host_args():
    """valid (host) pointers for every pointer argument: nothing is launched by the calls below, so nothing dereferences them"""
    buf = (ctypes.c_char * 512)()
    p = (ctypes.addressof(buf) + 63) & ~63
    return dict(grad=p, m=p + 64, v=p + 128, tensors=p + 192, chunks=p + 256, hyper=p + 320, step=p + 384, sq=p + 448), buf


def _call(h, a, algo=0, nchunks=1, **over):
    a = {**a, **over}
    return h.goat_optim_step(None, algo, a['grad'], a['m'], a['v'], a['tensors'], a['chunks'], nchunks, a['hyper'], a['step'], a['sq'])


def test_symbols_are_exported_and_bound():
    import os
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    for name in ('goat_optim_step', 'goat_optim_advance'):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['goat_optim_step']) == 11 and len(_lib.SIGNATURES['goat_optim_advance']) == 4
    assert ctypes.sizeof(_lib.OptimTensor) == 56 and ctypes.sizeof(_lib.OptimHyper) == 48          # the structs of include/goat_hip.h


def test_argument_validation_without_gpu():
    from vln_goat_amd import _lib
    h = _lib.lib()
    a, _keep = _host_args()
    E_ARG = -1
    for name in ('grad', 'tensors', 'chunks', 'hyper', 'step', 'sq'):
        for algo in (_lib.OPT_ADAMW, _lib.OPT_ADAM, _lib.OPT_RMSPROP, _lib.OPT_SGD):
            assert _call(h, a, algo, **{name: None}) == E_ARG, (name, algo)
    assert _call(h, a, _lib.OPT_ADAMW, m=None) == E_ARG and _call(h, a, _lib.OPT_ADAM, v=None) == E_ARG
    assert _call(h, a, _lib.OPT_RMSPROP, v=None) == E_ARG
    for algo in (-1, 4, 17):
        assert _call(h, a, algo) == E_ARG and _call(h, a, algo, nchunks=0) == E_ARG
    assert _call(h, a, _lib.OPT_ADAMW, nchunks=-1) == E_ARG
    for algo in (_lib.OPT_ADAMW, _lib.OPT_ADAM, _lib.OPT_RMSPROP, _lib.OPT_SGD):
        assert _call(h, a, algo, nchunks=0) == 0
    assert _call(h, a, _lib.OPT_RMSPROP, nchunks=0, m=None) == 0 and _call(h, a, _lib.OPT_SGD, nchunks=0, m=None, v=None) == 0     # moments they do not have
    assert h.goat_optim_advance(None, None, a['sq'], a['sq'] + 4) == E_ARG
    assert h.goat_optim_advance(None, a['step'], None, a['sq'] + 4) == E_ARG
    assert h.goat_optim_advance(None, a['step'], a['sq'], None) == E_ARG


def _cpu_case(algo='adamW', **kw):
    from vln_goat_amd import dp, optim
    torch.manual_seed(0)
    shapes = {'a.weight': (5, 3), 'a.bias': (5,), 'frozen.weight': (4,), 'unused.weight': (2, 2), 'b.weight': (7,)}
    params = {n: torch.nn.Parameter(torch.randn(s)) for n, s in shapes.items()}
    params['frozen.weight'].requires_grad_(False)
    usage = {id(p): (set() if n == 'unused.weight' else {'nav'}) for n, p in params.items()}
    arena = dp.GradArena(list(params.values()), usage).attach()
    return params, arena, optim.FusedTorchOptim(params.items(), arena, algo=algo, **kw)


def test_constructor_rejects_what_it_does_not_implement():
    from vln_goat_amd import optim
    params, arena, opt = _cpu_case()
    assert [opt.names[id(p)] for p in opt.params] == [n for n in ('a.weight', 'a.bias', 'b.weight')]
    ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-5).param_groups[0]
    assert set(opt.param_groups[0]) == set(ref) and len(opt.param_groups) == 1
    assert all(opt.param_groups[0][k] == ref[k] for k in ref if k != 'params')
    for bad in ('adamw', 'AdamW', 'lamb', None):
        with pytest.raises(ValueError):
            optim.FusedTorchOptim(params.items(), arena, algo=bad)
    for algo, kw in (('sgd', dict(momentum=0.9)), ('rms', dict(momentum=0.5)), ('rms', dict(centered=True)), ('adam', dict(amsgrad=True)),
                     ('adamW', dict(amsgrad=True)), ('sgd', dict(nesterov=True, momentum=0.9)), ('adamW', dict(lr=-1.0))):
        with pytest.raises(ValueError):
            optim.FusedTorchOptim(params.items(), arena, algo=algo, **kw)


@pytest.mark.parametrize('algo,cls', [('adamW', torch.optim.AdamW), ('adam', torch.optim.Adam), ('rms', torch.optim.RMSprop), ('sgd', torch.optim.SGD)])
def test_state_dict_interchanges_with_torch(algo, cls):
    """torch -> fused -> torch: two steps of torch's optimizer on CPU (the frozen and the unused parameter get no gradient, so torch keeps no
    state for them), loaded into the fused class, written out again and loaded into a fresh torch optimizer: moments and step exact."""
    params, arena, opt = _cpu_case(algo, lr=3e-4)
    assert opt.state_dict()['state'] == {}                          # nothing stepped yet
    plist = list(params.values())
    topt = cls(plist, lr=1e-3)
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        for n, p in params.items():
            p.grad = torch.randn(p.shape, generator=g) if n not in ('frozen.weight', 'unused.weight') else None
        topt.step()
    tsd = topt.state_dict()
    opt.load_state_dict(tsd)
    assert opt.param_groups[0]['lr'] == 1e-3                          # the group's hyper-parameters come with the checkpoint, as in torch
    sd = opt.state_dict()
    covered = [0, 1, 4]
    assert sd['param_groups'][0]['params'] == list(range(5))
    if algo == 'sgd':
        assert sd['state'] == {} and tsd['state'] == {}
    else:
        assert sorted(sd['state']) == covered == sorted(tsd['state'])
        for i in covered:
            assert list(sd['state'][i]) == list(tsd['state'][i])
            assert float(sd['state'][i]['step']) == 2.0 and type(sd['state'][i]['step']) is type(tsd['state'][i]['step'])
            for k, v in tsd['state'][i].items():
                if k != 'step':
                    assert torch.equal(sd['state'][i][k], v) and sd['state'][i][k].data_ptr() != v.data_ptr()
            assert opt.state_of(plist[i])['step'] == 2
    fresh = cls([torch.nn.Parameter(p.detach().clone()) for p in plist], lr=1.0)
    fresh.load_state_dict(sd)
    fsd = fresh.state_dict()
    assert sorted(fsd['state']) == sorted(tsd['state']) and fsd['param_groups'][0]['lr'] == 1e-3
    for i in fsd['state']:
        for k, v in tsd['state'][i].items():
            assert torch.equal(torch.as_tensor(fsd['state'][i][k]), torch.as_tensor(v)), (i, k)


def test_load_state_dict_accepts_old_checkpoints_and_refuses_mismatches():
    params, arena, opt = _cpu_case('adamW')
    plist = list(params.values())
    mk = lambda i, step: {'step': step, 'exp_avg': torch.full(plist[i].shape, 0.5, dtype=torch.float64), 'exp_avg_sq': torch.full(plist[i].shape, 0.25)}
    group = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=2e-5).param_groups[0], params=list(range(5)))
    opt.load_state_dict({'state': {i: mk(i, 7) for i in (0, 1, 4)}, 'param_groups': [group]})           # int steps (torch 1.9), float64 moments
    assert opt.steps_done() == 7 and opt.param_groups[0]['lr'] == 2e-5
    st = opt.state_of(plist[4])
    assert st['exp_avg'].dtype == torch.float32 and bool((st['exp_avg'] == 0.5).all()) and bool((st['exp_avg_sq'] == 0.25).all())
    assert float(opt.state_dict()['state'][1]['step']) == 7.0
    bad = {i: mk(i, 7) for i in (0, 1, 4)}
    bad[0]['exp_avg'] = torch.zeros(3, 5)
    with pytest.raises(ValueError, match='shape'):
        opt.load_state_dict({'state': bad, 'param_groups': [group]})
    uneven = {i: mk(i, 7) for i in (0, 1, 4)}
    uneven[1]['step'] = torch.tensor(6.0)
    with pytest.raises(ValueError, match='different number'):
        opt.load_state_dict({'state': uneven, 'param_groups': [group]})
    with pytest.raises(ValueError, match='different number'):
        opt.load_state_dict({'state': {i: mk(i, 7) for i in (0, 1)}, 'param_groups': [group]})              # one covered parameter never stepped
    with pytest.raises(ValueError):
        opt.load_state_dict({'state': {}, 'param_groups': [dict(group, params=list(range(4)))]})
    assert opt.steps_done() == 7                                       # a refused checkpoint leaves the optimizer as it was
    # entries of parameters outside the arena (index 2: frozen, 3: unused) are ignored
    extra = {i: mk(i, 3) for i in (0, 1, 4)}
    extra[3] = {'step': 9, 'exp_avg': torch.zeros(2, 2), 'exp_avg_sq': torch.zeros(2, 2)}
    opt.load_state_dict({'state': extra, 'param_groups': [group]})
    assert opt.steps_done() == 3 and sorted(opt.state_dict()['state']) == [0, 1, 4]


def test_build_nav_optimizers_mirrors_the_reference():
    import types
    from vln_goat_amd import dp, optim
    net, critic = torch.nn.Linear(4, 3), torch.nn.Linear(3, 1)
    arena = dp.GradArena(list(net.parameters()), {id(p): {'nav'} for p in net.parameters()}).attach()
    for name, cls in (('rms', torch.optim.RMSprop), ('adam', torch.optim.Adam), ('adamW', torch.optim.AdamW), ('sgd', torch.optim.SGD)):
        opt, copt = optim.build_nav_optimizers(types.SimpleNamespace(optim=name, lr=1e-5), net, critic, arena)
        assert isinstance(opt, optim.FusedTorchOptim) and opt.torch_class is cls and type(copt) is cls
        assert opt.param_groups[0]['lr'] == 1e-5 == copt.param_groups[0]['lr'] and len(opt.params) == 2
        copt.step()                                                    # no gradient: nothing moves, no state
        assert copt.state_dict()['state'] == {}
    with pytest.raises(ValueError):
        optim.build_nav_optimizers(types.SimpleNamespace(optim='lamb', lr=1e-5), net, critic, arena)
