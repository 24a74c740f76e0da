"""Construction order of the pre-training and the navigation model against tests/golden/module_tree_order.json
(tests/golden/make_module_tree_order.py holds the configurations and what is recorded): the ordered parameter and module names
and a hash of the seeded parameters.  The stems of both trees are one set of classes (encoders.py) whose constructors branch on
the tree; a sub-module created earlier, later or once more than before changes the order or the random draws, and fails here.
CPU only (module construction)."""
import importlib.util
import json
import os

import pytest

from helpers import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden')
_spec = importlib.util.spec_from_file_location('make_module_tree_order', os.path.join(GOLD, 'make_module_tree_order.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope='module')
def fixture():
    with open(os.path.join(GOLD, 'module_tree_order.json')) as f:
        return json.load(f)


def test_fixture_covers_every_configuration(fixture):
    assert sorted(fixture) == sorted('%s/%s' % c for c in gen.CASES)


@pytest.mark.parametrize('tree,tag', gen.CASES)
def test_module_tree_order(fixture, tree, tag):
    ref = fixture['%s/%s' % (tree, tag)]
    got = gen.record(gen.build(tree, tag))
    assert got['parameters'] == ref['parameters']       # lists: the order counts
    assert got['modules'] == ref['modules']
    assert got['sha256'] == ref['sha256']               # same random draws in the same sequence
