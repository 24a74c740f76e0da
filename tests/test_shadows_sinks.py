"""The two protocols of the op layer that run without a kernel, on CPU tensors: the weight-shadow cache (vln_goat_amd.shadows)
and the gradient-sink protocol (vln_goat_amd.gradsink), and hipops as the facade of both."""
import pytest
import torch


def _params():
    torch.manual_seed(3)
    q, k, v = (torch.nn.Parameter(torch.randn(4, 6)) for _ in range(3))
    bq, bk = (torch.nn.Parameter(torch.randn(4)) for _ in range(2))
    return q, k, v, bq, bk


def _accessors(q, k, v, bq, bk):
    """(owner, call, expected key, expected contents) of one use of each of the five accessors"""
    from vln_goat_amd import shadows
    bf = torch.bfloat16
    return [
        (q, lambda: shadows._shadow(q, bf), (bf, False, 0), lambda: q.detach().to(bf)),
        (q, lambda: shadows._shadow(q, torch.float32, True, 2), (torch.float32, True, 2),
         lambda: torch.nn.functional.pad(q.detach(), (0, 2)).t()),
        (q, lambda: shadows._shadow_cat((q, k, v), bf), ('cat', bf, False, (id(q), id(k), id(v))),
         lambda: torch.cat([q, k, v], 0).detach().to(bf)),
        (bq, lambda: shadows._cat_bias((bq, bk)), ('catb', (id(bq), id(bk))), lambda: torch.cat([bq, bk], 0).detach()),
        (bq, lambda: shadows._bias_padded(bq, 8), ('bpad', 8), lambda: torch.nn.functional.pad(bq.detach(), (0, 4))),
        (k, lambda: shadows._shadow_rows_padded(k, bf, 8), ('rowpad', bf, 8),
         lambda: torch.nn.functional.pad(k.detach(), (0, 0, 0, 4)).to(bf)),
    ]


def test_shadow_keys_are_the_documented_tuples():
    """optim._copies and tests/test_train_step_gpu.py read these tuples: they are the literal ones of shadows.py's table"""
    q, k, v, bq, bk = _params()
    want = {}
    for owner, call, key, ref in _accessors(q, k, v, bq, bk):
        t = call()
        assert torch.equal(t, ref()) and t.is_contiguous(), key
        want.setdefault(id(owner), (owner, set()))[1].add(key)
    for owner, keys in want.values():
        assert set(owner.__dict__['_goat_shadow']) == keys
    assert '_goat_shadow' not in v.__dict__ and '_goat_shadow' not in bk.__dict__      # a concatenated copy hangs off its first member
    bf = torch.bfloat16
    assert set(q.__dict__['_goat_shadow']) == {(bf, False, 0), (torch.float32, True, 2), ('cat', bf, False, (id(q), id(k), id(v)))}
    assert set(bq.__dict__['_goat_shadow']) == {('catb', (id(bq), id(bk))), ('bpad', 8)}
    assert set(k.__dict__['_goat_shadow']) == {('rowpad', bf, 8)}


def test_a_stale_shadow_is_rebuilt_into_its_own_storage():
    q, k, v, bq, bk = _params()
    acc = _accessors(q, k, v, bq, bk)
    before = [(call(), call().data_ptr()) for _, call, _, _ in acc]
    for (_, call, key, _), (t, ptr) in zip(acc, before):
        assert call() is t, key                       # a hit returns the cached object
    with torch.no_grad():
        for p in (q, k, v, bq, bk):
            p.mul_(-1.5).add_(0.25)                   # in-place: the version counters move
    for (_, call, key, ref), (t, ptr) in zip(acc, before):
        now = call()
        assert now is t and now.data_ptr() == ptr, key
        assert torch.equal(now, ref()), key


def test_refresh_shadows_rebuilds_in_place_skips_done_and_drops_orphans():
    from vln_goat_amd import hipops, shadows
    q, k, v, bq, bk = _params()
    acc = _accessors(q, k, v, bq, bk)
    held = [call() for _, call, _, _ in acc]
    ptrs = [t.data_ptr() for t in held]
    by_id = {id(p): p for p in (q, k, v, bq, bk)}
    for p in (q, k, v, bq, bk):
        p.data.mul_(2.0)                              # raw write: no version bump, the accessors still return the stale copies
    assert all(call() is t and not torch.equal(t, ref()) for (_, call, _, ref), t in zip(acc, held))
    skip = shadows._shadow(q, torch.bfloat16)
    stale = skip.clone()
    assert hipops.refresh_shadows(q, by_id, done={skip.data_ptr()}) == 2      # q's three copies minus the one in `done`
    assert torch.equal(skip, stale)
    assert hipops.refresh_shadows(q, by_id) == 3
    assert hipops.refresh_shadows(bq, by_id) == 2 and hipops.refresh_shadows(k, by_id) == 1
    assert hipops.refresh_shadows(v, by_id) == 0                               # nothing hangs off a non-first member
    for (_, call, key, ref), t, ptr in zip(acc, held, ptrs):
        assert call() is t and t.data_ptr() == ptr and torch.equal(t, ref()), key
    # a member of a concatenated copy is gone: the entry is deleted, the others are rebuilt and counted
    del by_id[id(k)], by_id[id(bk)]
    assert hipops.refresh_shadows(q, by_id) == 2 and hipops.refresh_shadows(bq, by_id) == 1
    assert not [key for key in q.__dict__['_goat_shadow'] if key[0] == 'cat']
    assert set(bq.__dict__['_goat_shadow']) == {('bpad', 8)}


class _Arena:
    """fake gradient-arena slices on CPU tensors: what dp.GradArena.attach leaves on a parameter"""

    def __init__(self, *params, unbound=()):
        from vln_goat_amd import gradsink
        from vln_goat_amd.wgrad_queue import WgradQueue
        assert not WgradQueue.pending_ids
        gradsink.ARENA_EPOCH[0] += 1                  # a new step
        self.sinks = {}
        for p in params:
            s = torch.full_like(p, 7.0).detach()      # stale values of the previous step
            self.sinks[id(p)] = s
            if not any(p is u for u in unbound):
                p.__dict__['_goat_sink'] = s
                p.grad = s
            p.__dict__.pop('_goat_epoch', None)

    def stale(self, p):
        return bool((self.sinks[id(p)] == 7.0).all())

    def clear(self, p):
        return bool((self.sinks[id(p)] == 0.0).all())


def test_first_touch_clears_exactly_the_unwritten_slices_of_a_mixed_set():
    from vln_goat_amd import gradsink
    q, k, v, bq, bk = _params()
    ar = _Arena(q, k, v, bq)
    bq.__dict__['_goat_prezero'] = True               # small parameter: cleared at the start of the step, never a first touch
    assert gradsink._first_touch(k) is True and ar.stale(k)      # sole writer, first in the step: it will overwrite, nothing is cleared
    ar.sinks[id(k)].fill_(3.0)                        # ... k's gradient is written
    assert gradsink._first_touch(q, k, v, bq) is False           # mixed: k written, q and v not
    assert ar.clear(q) and ar.clear(v) and bool((ar.sinks[id(k)] == 3.0).all()) and ar.stale(bq)
    assert gradsink._first_touch(q, k, v) is False and gradsink._first_touch(bq) is False
    gradsink.ARENA_EPOCH[0] += 1
    assert gradsink._first_touch(q, k, v) is True                # the next step: all first again, nothing to clear
    assert bool((ar.sinks[id(k)] == 3.0).all())


def test_prep_fallback_clears_once_and_marks_the_slice_written():
    from vln_goat_amd import gradsink
    q, k, v, bq, bk = _params()
    ar = _Arena(q, k, unbound=(k,))
    gradsink._prep_fallback(q, k, None)
    assert ar.clear(q) and ar.stale(k)                # k has no bound sink: autograd owns its .grad
    assert gradsink._first_touch(q) is False          # "not first": the fallback's autograd add must not be overwritten
    ar.sinks[id(q)].fill_(5.0)
    gradsink._prep_fallback(q)
    assert bool((ar.sinks[id(q)] == 5.0).all())


def test_small_sinks_is_all_or_nothing():
    from vln_goat_amd import gradsink
    q, k, v, bq, bk = _params()
    ar = _Arena(q, bq, k, unbound=(k,))
    assert gradsink.small_sinks((q, bq, k)) is None   # one parameter without a sink: every gradient goes back to autograd ...
    assert ar.clear(q) and ar.clear(bq) and ar.stale(k)          # ... which adds into .grad: the stale slices are cleared
    assert gradsink._first_touch(q) is False and gradsink._first_touch(bq) is False
    ar = _Arena(q, bq)
    sinks = gradsink.small_sinks((q, bq))
    assert len(sinks) == 2 and sinks[0] is ar.sinks[id(q)] and sinks[1] is ar.sinks[id(bq)]
    assert ar.clear(q) and ar.clear(bq)               # first write of the step: cleared, the kernel adds
    sinks[0].fill_(2.0)
    assert gradsink.small_sinks((q, bq))[0] is sinks[0] and bool((sinks[0] == 2.0).all())      # second use in the step: accumulate
    q.grad = None                                     # unbinding .grad restores the autograd path
    assert gradsink._sink(q) is None and gradsink.small_sinks((q, bq)) is None


_FACADE = {
    'shadows': ['_shadow', '_shadow_cat', '_cat_bias', '_bias_padded', '_shadow_rows_padded', 'refresh_shadows', '_store_shadow'],
    'gradsink': ['_sink', '_sink_cat', 'ARENA_EPOCH', '_first_touch', '_prep_fallback', 'small_sinks'],
}


@pytest.mark.parametrize('module', sorted(_FACADE))
def test_hipops_is_a_facade_of_the_shadow_and_sink_modules(module):
    import importlib
    from vln_goat_amd import hipops
    home = importlib.import_module('vln_goat_amd.' + module)
    for name in _FACADE[module]:
        assert getattr(hipops, name) is getattr(home, name), name
        if callable(getattr(home, name)):
            assert getattr(home, name).__module__ == 'vln_goat_amd.' + module, name


def test_arena_epoch_is_the_list_first_touch_reads():
    """dp.GradArena.zero() bumps hipops.ARENA_EPOCH[0]: it must be the object _first_touch looks at"""
    from vln_goat_amd import gradsink, hipops
    assert hipops.ARENA_EPOCH is gradsink.ARENA_EPOCH and hipops.ARENA_EPOCH is gradsink._first_touch.__globals__['ARENA_EPOCH']
    assert callable(hipops.linear_wgrad) and callable(hipops.wgrad) and not hasattr(hipops, '_wgrad_impl')
    q = torch.nn.Parameter(torch.zeros(2, 2))
    _Arena(q)
    assert gradsink._first_touch(q) is True and gradsink._first_touch(q) is False
    hipops.ARENA_EPOCH[0] += 1
    assert gradsink._first_touch(q) is True


def test_fused_adamw_copies_reads_the_shadow_keys():
    """optim._copies on cached copies of every kind: which copies the update kernel refreshes itself (their addresses, in
    the parameters' element order) and which are left to refresh_shadows — the slot rules of the kernel's per-tensor record (two bf16
    images or one K-padded + one bf16, one float32 image)."""
    from vln_goat_amd import optim, shadows
    torch.manual_seed(1)
    q, k, v = (torch.nn.Parameter(torch.randn(8, 16)) for _ in range(3))
    bq, bk, bv = (torch.nn.Parameter(torch.randn(8)) for _ in range(3))
    w7 = torch.nn.Parameter(torch.randn(8, 7))
    bf = torch.bfloat16
    plain, qkv = shadows._shadow(q, bf), shadows._shadow_cat((q, k, v), bf)
    transposed, f32 = shadows._shadow(q, bf, True), shadows._shadow(q, torch.float32)       # not the kernel's: left to refresh_shadows
    kv, k_plain, k_rows = shadows._shadow_cat((k, v), bf), shadows._shadow(k, bf), shadows._shadow_rows_padded(k, bf, 64)
    biases, b_padded = shadows._cat_bias((bq, bk, bv)), shadows._bias_padded(bq, 64)
    padded = shadows._shadow(w7, bf, False, 1)
    slots, done = optim._copies([q, k, v, bq, bk, bv, w7])
    # k: the kv image takes its first slot, the plain one its second (cache order: k's own entries, after q's qkv image was weighed
    # and refused for want of a third slot on k) — whatever the order, every copy in `done` is completely covered by slots
    assert plain.data_ptr() in done and padded.data_ptr() in done and biases.data_ptr() in done
    assert transposed.data_ptr() not in done and f32.data_ptr() not in done and b_padded.data_ptr() not in done
    assert slots[id(q)]['bf16'][0] == plain.data_ptr() and slots[id(w7)]['pad'] == (padded.data_ptr(), 7, 8)
    assert [slots[id(b)]['f32'] for b in (bq, bk, bv)] == [biases.data_ptr() + 32 * i for i in range(3)]
    covered = {p for sl in slots.values() for p in sl['bf16']}
    for t, members in ((qkv, (q, k, v)), (kv, (k, v))):
        rows = [t.data_ptr() + 2 * 16 * 8 * i for i in range(len(members))]
        assert (t.data_ptr() in done) == all(r in slots[id(m)]['bf16'] for r, m in zip(rows, members))
    assert all(len(sl['bf16']) <= (1 if sl['pad'] is not None else 2) for sl in slots.values())
    assert len([t for t in (qkv, kv, k_plain, k_rows) if t.data_ptr() in done]) == 2          # k has two bf16 slots for four images
    assert covered >= {plain.data_ptr()}
