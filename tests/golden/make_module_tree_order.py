"""Construction order of the two model trees, written as a fixture (imports only this package; CPU):

    python tests/golden/make_module_tree_order.py    -> tests/golden/module_tree_order.json

For every configuration below the model is built after `torch.manual_seed(0)`, and the fixture records the ORDERED
`named_parameters()` and `named_modules()` names and a SHA-256 over the parameter bytes in that order.  The registration order of
the sub-modules decides the first two; constructing a module draws random numbers before `init_weights()` runs, so the hash pins
the sequence of constructions too.  (contract_*.json pins names and shapes against the reference, order-independent; this pins
the order, against this package's own history.)  tests/test_module_tree_order.py rebuilds the same models and compares.
"""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# one layer of each kind, vocabulary 300: the order of construction does not depend on the sizes
SMALL = dict(num_l_layers=1, num_top_layer=1, num_pano_layers=1, vocab_size=300)
PRETRAIN = {
    'r2r': {},
    'bacl_type1_xattn': dict(do_back_txt=True, do_back_txt_type='type_1', z_cross_attn=True),
    'bacl_type2_door_xattn': dict(do_back_txt=True, do_back_txt_type='type_2', do_add_method='door', z_cross_attn=True, do_front_txt=True),
    'reverie': dict(name='REVERIE', obj_feat_size=768, obj_prob_size=100, image_prob_size=100, obj_name_vocab_size=45, use_obj_name=True,
                    pretrain_tasks=['mlm', 'mrc', 'sap', 'og', 'cfp']),
    'no_cfp': dict(pretrain_tasks=['mlm', 'sap']),
}
NAV_SMALL = dict(num_l_layers=1, num_x_layers=1, num_pano_layers=1, vocab_size=300, dropout=0.1, feat_dropout=0.5, mode='train')
ALL_ON = dict(do_back_img=True, do_back_txt=True, do_front_img=True, do_front_his=True, do_front_txt=True)
NAV = {
    # the two configurations of tests/test_boundary_contract.py
    'r2r': dict(ALL_ON, do_back_txt_type='type_2', do_back_img_type='type_1', do_add_method='door'),
    'reverie': dict(ALL_ON, do_back_txt_type='type_2', do_back_img_type='type_1', do_add_method='door', dataset='reverie', obj_feat_size=768),
    'causal_off': {},
    'type1_txt_type2_img_concat': dict(ALL_ON, do_back_txt_type='type_1', do_back_img_type='type_2', do_add_method='concat'),
    'extract_cfp': dict(mode='extract_cfp_features'),
}
CASES = [('pretrain', k) for k in PRETRAIN] + [('nav', k) for k in NAV]


def build(tree, tag):
    from vln_goat_amd import config as gcfg, nav_model, pretrain_model
    if tree == 'pretrain':
        cfg = gcfg.make_config(**{**SMALL, **PRETRAIN[tag]})
        torch.manual_seed(0)
        return pretrain_model.GlocalTextPathCMTPreTraining(cfg)
    cfg = nav_model.nav_config_from_args(SimpleNamespace(**{**NAV_SMALL, **NAV[tag]}))
    torch.manual_seed(0)
    return nav_model.GlocalTextPathNavCMT(cfg)


def record(model):
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().contiguous().numpy().tobytes())
    return {'parameters': [n for n, _ in model.named_parameters()], 'modules': [n for n, _ in model.named_modules()],
            'sha256': h.hexdigest()}


if __name__ == '__main__':
    out = {'%s/%s' % c: record(build(*c)) for c in CASES}
    with open(os.path.join(HERE, 'module_tree_order.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print('wrote module_tree_order.json', {k: (len(v['parameters']), v['sha256'][:12]) for k, v in out.items()})
