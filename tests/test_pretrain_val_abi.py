"""goat_val_rows / goat_val_cfp / goat_val_reduce and pretrain_eval checks that need no GPU: the entries' error codes (returned before
any launch), `validate`'s dispatch and training-flag handling on the host, and the cross-rank sum of the accumulator over gloo."""
import ctypes
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

E_ARG, E_SHAPE = -1, -2


def _handle():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_val_rows_error_codes_without_a_launch():
    h = _handle()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    #     stream logits ld M  N  labels soft ld_soft row_loss row_hit
    hard = [None, p, 8, 2, 8, p, None, 0, p, p]
    soft = [None, p, 8, 2, 8, None, p, 8, p, p]
    for ok in (hard, soft):
        for k in (1, 8, 9):                                     # logits, row_loss, row_hit
            a = list(ok)
            a[k] = None
            assert h.goat_val_rows(*a) == E_ARG, k
        for k, v in ((3, 0), (3, -2), (4, 0), (4, -1), (2, 7), (2, 0)):      # M < 1, N < 1, ld < N
            a = list(ok)
            a[k] = v
            assert h.goat_val_rows(*a) == E_SHAPE, (k, v)
    for labels, st in ((p, p), (None, None)):                   # both and neither of labels / soft
        a = list(hard)
        a[5], a[6], a[7] = labels, st, 8
        assert h.goat_val_rows(*a) == E_ARG
    for v in (7, 0, -8):                                        # ld_soft < N
        a = list(soft)
        a[7] = v
        assert h.goat_val_rows(*a) == E_SHAPE, v
    a = list(hard)
    a[7] = 0                                                    # (ld_soft is not looked at without soft targets)
    a[1], a[3] = None, 0                                        # a null pointer wins over a bad shape
    assert h.goat_val_rows(*a) == E_ARG


def test_val_cfp_error_codes_without_a_launch():
    h = _handle()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    xs = (ctypes.c_void_p * 3)(p, p, p)
    #    stream x  txt B  H  temperature row_loss row_hit
    ok = [None, xs, p, 4, 8, 0.5, p, p]
    for k in (1, 2, 6, 7):
        a = list(ok)
        a[k] = None
        assert h.goat_val_cfp(*a) == E_ARG, k
    for hole in range(3):                                       # a null pointer inside the table of three
        a = list(ok)
        a[1] = (ctypes.c_void_p * 3)(*[None if j == hole else p for j in range(3)])
        assert h.goat_val_cfp(*a) == E_ARG, hole
    for k, v in ((3, 0), (3, -1), (3, 1025), (3, 1 << 20), (4, 0), (4, -3), (5, 0.0), (5, -1.0)):      # B < 1, B > 1024, H < 1, temperature
        a = list(ok)
        a[k] = v
        assert h.goat_val_cfp(*a) == E_SHAPE, (k, v)
    a = list(ok)
    a[2], a[3] = None, 0
    assert h.goat_val_cfp(*a) == E_ARG


def test_val_reduce_error_codes_without_a_launch():
    h = _handle()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    #    stream row_loss row_hit labels M acc
    ok = [None, p, p, None, 4, p]
    for k in (1, 2, 5):
        a = list(ok)
        a[k] = None
        assert h.goat_val_reduce(*a) == E_ARG, k
    for v in (0, -5):
        a = list(ok)
        a[4] = v
        assert h.goat_val_reduce(*a) == E_SHAPE, v
    a = list(ok)
    a[5], a[4] = None, 0
    assert h.goat_val_reduce(*a) == E_ARG


def test_ops_refuse_cpu_tensors():
    from vln_goat_amd import hipops, pretrain_eval
    loss, hit = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        hipops.val_rows(torch.zeros(4, 8), loss, hit, labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        hipops.val_cfp(*[torch.zeros(1, 8)] * 4, 0.5, loss, hit)
    with pytest.raises(RuntimeError):
        hipops.val_reduce(loss, hit, None, torch.zeros(3, dtype=torch.float64))
    st = pretrain_eval.ValStats(('a',), device='cpu')
    with pytest.raises(RuntimeError):
        st.add_rows('a', torch.zeros(4, 8), labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        st.add_rows('a', torch.zeros(4, 8))                     # neither labels nor soft
    st.add_rows('a', torch.zeros(0, 8), labels=torch.zeros(0, dtype=torch.int64))      # an empty selection launches nothing
    assert st.read() == {'a': (0.0, 0.0, 0.0)}
    with pytest.raises(ValueError):
        pretrain_eval.ValStats(('a', 'a'))


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


@pytest.mark.parametrize('training', [True, False])
def test_validate_on_the_host(training):
    from vln_goat_amd import pretrain_eval
    model = _Tiny().train(training)
    logs, best, flag = pretrain_eval.validate(model, {}, setname='_unseen', max_metrix=0.25)
    assert logs == {} and best == 0.25 and flag is False and model.training is training
    with pytest.raises(ValueError):
        pretrain_eval.validate(model, {'itm': []})
    assert model.training is training                            # put back on the way out of the error as well


def test_validate_dispatch_and_the_best_checkpoint_rule(monkeypatch):
    """the dispatch by prefix, the key names and the `facc >= max_metrix` rule, with the five loops replaced by stand-ins"""
    from vln_goat_amd import pretrain_eval
    seen = []

    def stand_in(name, log):
        def f(model, loader, *rest):
            assert not model.training
            seen.append((name, loader) + rest)
            return dict(log)
        return f

    glf = {'gloss': 1.0, 'lloss': 2.0, 'floss': 3.0, 'gacc': 0.5, 'lacc': 0.25, 'facc': 0.75, 'tok_per_s': 9.0}
    for name, log in (('mlm', {'loss': 1.0, 'acc': 0.5, 'tok_per_s': 2.0}), ('mrc', {'loss': 1.0, 'acc': 0.5, 'feat_per_s': 2.0}),
                      ('og', {'loss': 1.0, 'acc': 0.5, 'tok_per_s': 2.0}), ('sap', glf), ('cfp', glf)):
        monkeypatch.setattr(pretrain_eval, 'validate_' + name, stand_in(name, log))
    model = _Tiny().train()
    loaders = {'mlm': 'L0', 'mrc_1': 'L1', 'sap': 'L2', 'og': 'L3', 'cfp': 'L4'}
    logs, best, flag = pretrain_eval.validate(model, loaders, setname='_unseen', max_metrix=0.75, tem=0.07)
    assert seen == [('mlm', 'L0'), ('mrc', 'L1'), ('sap', 'L2'), ('og', 'L3'), ('cfp', 'L4', 0.07)]
    assert model.training and (best, flag) == (0.75, True)       # >=: an equal facc is a new best, as in the reference
    want = {'val_unseen_mlm_%s' % k for k in ('loss', 'acc', 'tok_per_s')} | {'val_unseen_mrc_1_%s' % k for k in ('loss', 'acc', 'feat_per_s')} \
        | {'val_unseen_og_%s' % k for k in ('loss', 'acc', 'tok_per_s')} | {'val_unseen_%s_%s' % (t, k) for t in ('sap', 'cfp') for k in glf}
    assert set(logs) == want and logs['val_unseen_sap_facc'] == 0.75
    assert pretrain_eval.validate(model, loaders, setname='_unseen', max_metrix=0.8, tem=0.07)[1:] == (0.8, False)
    assert pretrain_eval.validate(model, loaders, setname='_seen', max_metrix=0.1, tem=0.07)[1:] == (0.1, False)      # the unseen split only
    assert pretrain_eval.validate(model, loaders, setname='_unseen', tem=0.07)[1:] == (None, False)


# ---- the cross-rank sum (gloo, CPU), spawned as tests/test_dp_gloo.py spawns its ranks
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _filled(rank):
    """a hand-filled accumulator of two slots: loss sums with fractions, whole-number counts, one of them past 2^24"""
    return torch.tensor([[1.5 + rank, 3.0 + rank, 7.0], [0.125 * (rank + 1), 2.0 ** 24 + 1 + rank, 2.0 ** 25]], dtype=torch.float64)


def _worker_reduce(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from vln_goat_amd import pretrain_eval
    acc = _filled(rank)
    out = pretrain_eval.reduce_stats(acc)
    st = pretrain_eval.ValStats(('a', 'b'), device='cpu')       # read() goes through the same step
    st.acc.copy_(_filled(rank))
    q.put((rank, out is acc, out.numpy().copy(), st.read()))     # (numpy payloads are pickled by value)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_reduce_returns_the_sums_on_both_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_reduce, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in ps]
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    [p.join(60) for p in ps]
    want = _filled(0) + _filled(1)
    assert want[1, 1] == 2.0 ** 25 + 3                           # (exact in a double; a float32 sum would round it)
    for rank, same, got, read in res:
        assert same, rank                                        # in place
        assert (torch.from_numpy(got) == want).all(), (rank, got)
        assert read == {'a': tuple(want[0].tolist()), 'b': tuple(want[1].tolist())}, rank


def test_reduce_without_a_process_group_is_the_identity():
    from vln_goat_amd import pretrain_eval
    acc = _filled(0)
    assert pretrain_eval.reduce_stats(acc) is acc and (acc == _filled(0)).all()
