"""The validation-metrics fixture (tests/golden/nav_metrics.npz / .json, written by tests/golden/make_golden_metrics.py) as the tests of
goat_nav_metrics and evaluate.NavEvaluator read it."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    z = dict(np.load(os.path.join(HERE, 'golden', 'nav_metrics.npz'), allow_pickle=False))
    with open(os.path.join(HERE, 'golden', 'nav_metrics.json')) as f:
        ids = json.load(f)
    return z, ids


def fixture_scans(z, ids):
    from vln_goat_amd import rollout
    scans = []
    for k, sc in enumerate(ids['scans']):
        vp = sc['vpids']
        scans.append(rollout.ScanGraph(sc['name'], vp, z['pos_%d' % k], [(vp[a], vp[b]) for a, b in z['edges_%d' % k]]))
    return scans
