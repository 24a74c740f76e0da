"""helpers.clip_adamw_step — the torch restatement of clip_grad_norm_(5.0) + the reference's AdamW that the GPU tests compare the fused
update with — against the trace the reference optimizer itself wrote (tests/golden/adamw_trace.npz, tests/golden/make_contract.py)."""
import numpy as np
import torch

from helpers import clip_adamw_step, load_golden

NO_DECAY = ('bias', 'LayerNorm.bias', 'LayerNorm.weight')


def test_restatement_reproduces_the_reference_trace_bit_for_bit():
    """All 7 tensors after each of the 3 steps (a clipped one, a tensor without any gradient, one that skips a step, a changing learning
    rate, decay on matrices only), and the moments after the last: equal, not close."""
    tr = load_golden('adamw_trace')
    names = [str(n) for n in tr['names']]
    params = {n: torch.from_numpy(tr['p0_' + n].copy()) for n in names}
    wd = {n: 0.0 if any(nd in n for nd in NO_DECAY) else 0.01 for n in names}
    state, checked = {}, 0
    for step in range(3):
        grads = {n: torch.from_numpy(tr['g%d_%s' % (step, n)].copy()) for n in names if ('g%d_%s' % (step, n)) in tr}
        # the recorded float32 norm goes in: which float32 sum of 28 000 squares torch forms depends on the CPU's vector unit, and the clipped
        # step's coefficient has to be the trace's to the bit.  The helper's own norm: the bound the device norm has against this trace.
        ref_norm = float(tr['gnorm%d' % step][0])
        own = clip_adamw_step({n: p.clone() for n, p in params.items()}, grads, {}, float(tr['lr'][step]), wd)
        assert abs(own - ref_norm) <= 1e-4 * ref_norm, (step, own, ref_norm)
        assert clip_adamw_step(params, grads, state, float(tr['lr'][step]), wd, norm=ref_norm) == ref_norm
        for n in names:
            assert np.array_equal(params[n].numpy(), tr['p%d_%s' % (step + 1, n)]), (step, n)
            checked += 1
    assert checked == 21
    assert sorted(state) == sorted(n for n in names if ('m_' + n) in tr) and 'unused.weight' not in state
    for n, st in state.items():
        assert np.array_equal(st['exp_avg'].numpy(), tr['m_' + n]) and np.array_equal(st['exp_avg_sq'].numpy(), tr['v_' + n]), n
    assert state['head.weight']['step'] == 2 and state['emb.word.weight']['step'] == 3
