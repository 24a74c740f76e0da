"""goat_nav_metrics (csrc/navmetrics.hip) and evaluate.NavEvaluator on the device against the IMPORTED REFERENCE's `_eval_item` /
`eval_metrics` (tests/golden/nav_metrics.npz from tests/golden/make_golden_metrics.py: networkx tables of three synthetic scans, items
of every (P, R) around the wave width and the diagonal count, backtracks, interleaved scans, REVERIE goal sets).

Bounds.  Columns 0 nav_error, 1 oracle_error, 2 trajectory_steps, 5 success, 6 oracle_success and 8 DTW are table values, exact minima,
counts, comparisons, and — DTW — one add per cell over exact minima in the reference's own order: BIT-equal.  Columns 3, 4, 7, 9, 10, 11
hold sums of at most 256 non-negative doubles taken in another order than numpy's (relative deviation <= 256 * 2^-53 = 3e-14) and `exp`
(a few ulp): within 1e-12 * max(1, |ref|).  The fixture's own reversed-order restatement deviates by about 1e-15 (recorded in the json,
asserted < 1e-13 by the generator and by tests/test_nav_metrics_abi.py)."""
import numpy as np
import pytest
import torch

from metrics_fixture import fixture, fixture_scans

pytestmark = pytest.mark.gpu

EXACT, SUMMED = (0, 1, 2, 5, 6, 8), (3, 4, 7, 9, 10, 11)
_CASE = {}


def case():
    """fixture, scans, and the fixture's networkx tables on the device (built once, never modified)"""
    if not _CASE:
        from vln_goat_amd import evaluate
        z, ids = fixture()
        scans = fixture_scans(z, ids)
        tables = {sc.name: z['dist_%d' % k] for k, sc in enumerate(scans)}
        _CASE.update(z=z, ids=ids, scans=scans, tables=tables, sd=evaluate.ScanDistances(scans, 'cuda', tables=tables))
    return _CASE


def check(got, ref, what=''):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for c in EXACT:
        same = got[:, c].view(np.int64) == ref[:, c].view(np.int64)
        assert same.all(), (what, 'column', c, 'items', np.nonzero(~same)[0][:8].tolist(), got[~same, c][:4], ref[~same, c][:4])
    for c in SUMMED:
        err = np.abs(got[:, c] - ref[:, c])
        ok = (err <= 1e-12 * np.maximum(1.0, np.abs(ref[:, c]))) | (np.isnan(got[:, c]) & np.isnan(ref[:, c]))
        print('%s column %d: max |err| %.3e' % (what, c, float(np.nanmax(err, initial=0.0))))
        assert ok.all(), (what, 'column', c, 'items', np.nonzero(~ok)[0][:8].tolist(), got[~ok, c][:4], ref[~ok, c][:4])


def arrays(z, items=None):
    """the CSR arrays of the fixture, or of a selection (with repeats) of its items"""
    if items is None:
        return z['item_scan'], z['pred'], z['pred_start'], z['ref'], z['ref_start']
    seg = lambda flat, start: [flat[start[i]:start[i + 1]] for i in items]
    p, r = seg(z['pred'], z['pred_start']), seg(z['ref'], z['ref_start'])
    csr = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    return z['item_scan'][list(items)], np.concatenate(p), csr(p), np.concatenate(r), csr(r)


def test_kernel_matches_the_reference_items():
    from vln_goat_amd import evaluate
    c = case()
    z = c['z']
    got = evaluate.nav_metrics(c['sd'], *arrays(z)).cpu().numpy()
    check(got, z['ref_cols'], 'fixture')
    assert np.isnan(got[:, 11]).sum() == np.isnan(z['ref_cols'][:, 11]).sum() >= 1          # the one-node reference path: 0 / 0
    lens = set(zip(np.diff(z['pred_start']).tolist(), np.diff(z['ref_start']).tolist()))
    assert {(1, 1), (1, 5), (2, 2), (7, 6), (63, 5), (64, 64), (65, 64), (130, 65), (40, 200)} <= lens
    # the LDS sized for longer reference paths than any item has: same bits
    wide = evaluate.nav_metrics(c['sd'], *arrays(z), max_ref=2047).cpu().numpy()
    assert np.array_equal(wide.view(np.int64), got.view(np.int64))


def test_single_items_and_three_thousand():
    from vln_goat_amd import evaluate
    c = case()
    z = c['z']
    N = len(z['item_scan'])
    for n in range(N):                                             # N = 1, every item on its own
        got = evaluate.nav_metrics(c['sd'], *arrays(z, [n])).cpu().numpy()
        check(got, z['ref_cols'][n:n + 1], 'item %d alone' % n)
    items = [(7 * k) % N for k in range(3000)]                      # the fixture tiled (7 and N = 22 are coprime: every item, scans interleaved)
    got = evaluate.nav_metrics(c['sd'], *arrays(z, items)).cpu().numpy()
    check(got, z['ref_cols'][items], 'N = 3000')


def test_strict_margin_at_exactly_three():
    from vln_goat_amd import evaluate
    c = case()
    z = c['z']
    at = np.nonzero(z['ref_cols'][:, 0] == 3.0)[0]
    assert len(at) >= 1
    got = evaluate.nav_metrics(c['sd'], *arrays(z)).cpu().numpy()
    assert (got[at, 0] == 3.0).all() and (got[at, 5] == 0.0).all() and (got[at, 7] == 0.0).all() and (got[at, 10] == 0.0).all()
    up = evaluate.nav_metrics(c['sd'], *arrays(z), margin=float(np.nextafter(3.0, 4.0))).cpu().numpy()
    assert (up[at, 5] == 1.0).all() and (up[at, 7] > 0.0).all()


def test_reverie_goal_rule():
    from vln_goat_amd import evaluate
    c = case()
    z = c['z']
    items = z['rv_items'].tolist()
    got = evaluate.nav_metrics(c['sd'], *arrays(z, items), goal=z['rv_goal'], goal_start=z['rv_goal_start']).cpu().numpy()
    assert set(np.diff(z['rv_goal_start']).tolist()) == {1, 4}
    assert np.array_equal(got[:, 5], z['rv_success']) and np.array_equal(got[:, 6], z['rv_oracle_success'])
    assert {0.0, 1.0} == set(got[:, 5].tolist()) and (got[:, 6] > got[:, 5]).any()
    assert np.array_equal(got[:, 2], z['rv_trajectory_steps'])
    for col, name in ((3, 'rv_trajectory_lengths'), (7, 'rv_spl')):
        assert (np.abs(got[:, col] - z[name]) <= 1e-12 * np.maximum(1.0, np.abs(z[name]))).all(), name
    # everything but the two success columns and what is formed from them is the R2R value of the same items
    ref = z['ref_cols'][items]
    for col in (0, 1, 2, 8):
        assert np.array_equal(got[:, col].view(np.int64), ref[:, col].view(np.int64)), col


def test_nav_evaluator_returns_the_reference_metrics():
    from vln_goat_amd import evaluate
    c = case()
    z, ids = c['z'], c['ids']
    close = lambda a, b: bool(np.all((np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) <= 1e-12 * np.maximum(1.0, np.abs(np.asarray(b, np.float64))))
                                     | (np.isnan(np.asarray(a, np.float64)) & np.isnan(np.asarray(b, np.float64)))))
    ev = evaluate.NavEvaluator(c['scans'], {k: tuple(v) for k, v in ids['gt_trajs'].items()}, tables=c['tables'])
    avg, metrics = ev.eval_metrics(ids['preds'])
    assert list(avg.keys()) == ids['avg_keys']
    for k, v in zip(ids['avg_keys'], z['avg_vals']):
        assert close(avg[k], v), (k, avg[k], v)
    want = ['action_steps'] + [n for n in ids['cols'] if n != 'gt_lengths'] + ['instr_id']
    assert sorted(metrics.keys()) == sorted(want)
    assert metrics['instr_id'] == [p['instr_id'] for p in ids['preds']]
    assert np.array_equal(np.asarray(metrics['action_steps'], np.float64), z['action_steps'])
    cols = np.zeros_like(z['ref_cols'])
    cols[:, 4] = z['ref_cols'][:, 4]
    for col, name in enumerate(ids['cols']):
        if name != 'gt_lengths':
            cols[:, col] = metrics[name]
    check(cols, z['ref_cols'], 'NavEvaluator')
    # REVERIE: the reference's eight averages, rgs / rgspl formed on the host
    rv = evaluate.NavEvaluator(c['scans'], {k: tuple(v) for k, v in ids['rv_gt_trajs'].items()}, obj2vps=ids['rv_obj2vps'], tables=c['tables'])
    ravg, rmetrics = rv.eval_metrics(ids['rv_preds'])
    assert list(ravg.keys()) == ids['rv_avg_keys'] and len(ravg) == 8
    for k, v in zip(ids['rv_avg_keys'], z['rv_avg_vals']):
        assert close(ravg[k], v), (k, ravg[k], v)
    assert sorted(rmetrics.keys()) == sorted(['action_steps', 'trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success', 'spl', 'rgs',
                                              'rgspl', 'instr_id'])
    for name in ('action_steps', 'trajectory_steps', 'success', 'oracle_success', 'rgs'):
        assert np.array_equal(np.asarray(rmetrics[name], np.float64), z['rv_' + name]), name
    for name in ('trajectory_lengths', 'spl', 'rgspl'):
        assert close(rmetrics[name], z['rv_' + name]), name
    assert 0 < sum(rmetrics['rgs']) < len(rmetrics['rgs'])
    # the package's own tables (scipy's Dijkstra) differ from networkx's in the last bits at most: the scores move by as little
    own = evaluate.NavEvaluator(c['scans'], {k: tuple(v) for k, v in ids['gt_trajs'].items()})
    avg2, _ = own.eval_metrics(ids['preds'])
    for k, v in zip(ids['avg_keys'], z['avg_vals']):
        assert np.isnan(v) or abs(avg2[k] - v) <= 1e-9 * max(1.0, abs(v)), (k, avg2[k], v)


def test_call_on_a_side_stream():
    from vln_goat_amd import evaluate
    c = case()
    z = c['z']
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = evaluate.nav_metrics(c['sd'], *arrays(z))
    side.synchronize()
    check(got.cpu().numpy(), z['ref_cols'], 'side stream')
