"""goat_nav_metrics / evaluate.NavEvaluator checks that need no GPU: the entry's error codes (returned before any launch), the
package's shortest-distance tables against the networkx tables of the fixture (tests/golden/make_golden_metrics.py), and the host-side
validation of NavEvaluator, which raises before anything touches a device."""
import ctypes
import os

import numpy as np
import pytest

from metrics_fixture import fixture, fixture_scans


def test_error_codes_without_a_launch():
    from vln_goat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    ok = [None, p, p, p, 1, p, p, p, p, p, None, None, 1, 4, 3.0, p]
    E_ARG, E_SHAPE = -1, -2
    for k in (1, 2, 3, 5, 6, 7, 8, 9, 15):                     # every pointer but stream / goal / goal_start
        a = list(ok)
        a[k] = None
        assert h.goat_nav_metrics(*a) == E_ARG, k
    for goal, goal_start in ((p, None), (None, p)):             # exactly one of the pair
        a = list(ok)
        a[10], a[11] = goal, goal_start
        assert h.goat_nav_metrics(*a) == E_ARG
    for k, v in ((12, 0), (12, -3), (4, 0), (13, 0), (13, 2048), (13, -1)):      # N, n_scans, max_ref
        a = list(ok)
        a[k] = v
        assert h.goat_nav_metrics(*a) == E_SHAPE, (k, v)
    a = list(ok)
    a[1], a[12] = None, 0                                       # a null pointer wins over a bad shape
    assert h.goat_nav_metrics(*a) == E_ARG


def test_scan_graph_shortest_matches_the_networkx_tables():
    z, ids = fixture()
    assert ids['reversed_order_max_rel_dev'] < 1e-13
    for k, sc in enumerate(fixture_scans(z, ids)):
        d, ref = sc.shortest()[0], z['dist_%d' % k]
        assert d.shape == ref.shape == (len(sc.vpids),) * 2
        assert np.isfinite(ref).all()
        assert (np.abs(d - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))).all(), (sc.name, float(np.abs(d - ref).max()))
    assert [len(s['vpids']) for s in ids['scans']] == [12, 33, 60]


def test_nav_evaluator_validates_on_the_host():
    from vln_goat_amd import evaluate
    z, ids = fixture()
    scans = fixture_scans(z, ids)
    gt = {k: tuple(v) for k, v in ids['gt_trajs'].items()}
    ev = evaluate.NavEvaluator(scans, gt, device='no-such-device')          # (a device is touched at the first launch only)
    good = ids['preds'][3]
    with pytest.raises(KeyError):
        ev.eval_metrics([dict(good, trajectory=good['trajectory'] + [['not_a_viewpoint']])])
    with pytest.raises(ValueError):
        ev.eval_metrics([dict(good, trajectory=[])])
    with pytest.raises(ValueError):
        ev.eval_metrics([dict(good, trajectory=[[]])])
    other = next(vp for vp in scans[ev._order[gt[good['instr_id']][0]]].vpids if vp != good['trajectory'][0][0])
    with pytest.raises(ValueError):
        ev.eval_metrics([dict(good, trajectory=[[other]] + good['trajectory'][1:])])
    with pytest.raises(KeyError):
        ev.eval_metrics([dict(good, instr_id='unknown_0')])
    with pytest.raises(ValueError):
        ev.eval_metrics([])
    assert ev._sd is None
    # the REVERIE form: an object without goal viewpoints is the reference's assert
    rgt = {k: tuple(v) for k, v in ids['rv_gt_trajs'].items()}
    rv = evaluate.NavEvaluator(scans, rgt, obj2vps={k: [] for k in ids['rv_obj2vps']}, device='no-such-device')
    with pytest.raises(ValueError):
        rv.eval_metrics(ids['rv_preds'][:1])
    assert rv._sd is None
