"""RxR-length instructions through the model trees: one pre-training step (mlm, sap, cfp) at 300 / 257 tokens against the CPU oracle,
and a navigation episode whose instruction batch is padded to 300 columns against the same batch padded to 200 (the kernels for
up to 256 keys).  Float32 1e-3, bfloat16 2e-2."""
import numpy as np
import pytest
import torch

from helpers import check_projections, oracle_run, projections

pytestmark = pytest.mark.gpu

WORD = 'bert.embeddings.word_embeddings.weight'


@pytest.fixture(scope='module')
def pretrain_case():
    """(config, seeded state dict, batch, {task: oracle loss vector and gradients}): one float32 oracle run per task, shared."""
    from vln_goat_amd import config as gcfg, pretrain_model, synth
    cfg = gcfg.make_config(num_l_layers=1, num_top_layer=1, num_pano_layers=1, vocab_size=600)
    model = pretrain_model.GlocalTextPathCMTPreTraining(cfg)
    sd = synth.seeded_state_dict(model, seed=3)
    batch = synth.make_pretrain_batch(B=2, T=[3, 2], L=[300, 257], seed=35, style='rich', vocab_size=600)
    refs = {task: oracle_run(cfg, {k: v.clone() for k, v in sd.items()}, batch, task) for task in ('mlm', 'sap', 'cfp')}
    return cfg, sd, batch, refs


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pretraining_step_at_300_tokens_matches_oracle(pretrain_case, dtype):
    import vln_goat_amd
    from vln_goat_amd import pretrain_model, synth
    cfg, sd, batch, refs = pretrain_case
    assert batch['txt_ids'].shape[1] == 300
    model = pretrain_model.GlocalTextPathCMTPreTraining(cfg)
    model.load_state_dict(sd)
    model.tie_weights()
    query = [n for n, _ in model.named_parameters() if n.endswith('attention.self.query.weight')][0]
    tol = 1e-3 if dtype == torch.float32 else 2e-2
    vln_goat_amd.set_compute_dtype(dtype)
    try:
        model = model.cuda().eval()
        gb = synth.batch_to(batch, 'cuda')
        for task in ('mlm', 'sap', 'cfp'):
            ref, ref_grads = refs[task]
            for p in model.parameters():
                p.grad = None
            loss = model(gb, task, compute_loss=True)
            loss.mean().backward()
            torch.cuda.synchronize()
            assert loss.shape == ref.shape
            err = float((loss.detach().float().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
            print('%s %s: loss error %.3e' % (task, dtype, err))
            assert err <= tol, (task, err)
            assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
            if dtype == torch.float32:
                # every element of the two gradients all 300 positions feed: seeded projections against the oracle's, at the relative
                # bound of the small-case float32 gradient check (1e-3 of the tensor's norm; 1e-3 of the largest norm for a tiny tensor)
                params = dict(model.named_parameters())
                gmax = max(float(g.norm()) for g in ref_grads.values() if g is not None)
                for n in (WORD, query):
                    rg = ref_grads[n]
                    assert rg is not None and params[n].grad is not None, n
                    check_projections(projections(params[n].grad), projections(rg), max(float(rg.double().norm()), 1e-3 * gmax), 1e-3,
                                      '%s %s' % (task, n))
    finally:
        vln_goat_amd.set_compute_dtype(torch.float32)


def _nav_model_and_episode():
    from types import SimpleNamespace
    from vln_goat_amd import nav_model, synth
    args = SimpleNamespace(num_l_layers=2, num_x_layers=2, num_pano_layers=2, dropout=0.5, feat_dropout=0.4, do_back_img=True, do_back_txt=True,
                           do_front_img=True, do_front_his=True, do_front_txt=True, vocab_size=1200, mode='train',
                           do_back_txt_type='type_2', do_back_img_type='type_1', do_add_method='door')
    model = nav_model.GlocalTextPathNavCMT(nav_model.nav_config_from_args(args))
    model.load_state_dict(synth.seeded_state_dict(model, seed=11))
    ep = synth.make_nav_episode(B=2, L=200, n_steps=1, seed=5, vocab_size=1200)
    lens = torch.tensor([200, 150])
    ep['txt_masks'] = torch.arange(200)[None, :] < lens[:, None]
    ep['txt_ids'] = torch.where(ep['txt_masks'], ep['txt_ids'].clamp_min(3), torch.ones_like(ep['txt_ids']))
    return model, ep


def test_navigation_step_is_invariant_to_padding_the_instruction_to_300():
    """Instructions of 200 and 150 tokens, padded once to 200 columns (goat_attn_fwd) and once to 300 (goat_attn_long_fwd).  The padding
    mask is -10000 and exp(-10000) = 0 in float32, so the language states at the valid positions and the logits of a navigation step are
    those of the narrower batch."""
    import vln_goat_amd
    from vln_goat_amd import synth
    model, ep = _nav_model_and_episode()
    wide = dict(ep)
    wide['txt_ids'] = torch.cat([ep['txt_ids'], torch.ones(2, 100, dtype=torch.int64)], 1)
    wide['txt_masks'] = torch.cat([ep['txt_masks'], torch.zeros(2, 100, dtype=torch.bool)], 1)
    vln_goat_amd.set_compute_dtype(torch.float32)
    model = model.cuda().eval()
    out = []
    with torch.no_grad():
        for e in (ep, wide):
            _, rec = synth.run_nav_episode(lambda m, b: model(m, b), e, device='cuda')
            out.append(rec)
    torch.cuda.synchronize()
    assert out[1]['txt_embeds'].shape[1] == 300
    valid = ep['txt_masks'].cuda()
    a = out[0]['txt_embeds'].float()[valid]
    b = out[1]['txt_embeds'].float()[:, :200][valid]
    err = float((a - b).abs().max() / a.abs().max())
    print('language states: %.3e' % err)
    assert err < 1e-3
    for k in ('global_logits', 'local_logits', 'fused_logits'):
        x, y = out[0]['steps'][0][k].float().cpu().numpy(), out[1]['steps'][0][k].float().cpu().numpy()
        assert np.array_equal(np.isinf(x), np.isinf(y)), k
        m = ~np.isinf(x)
        err = float(np.abs(x[m] - y[m]).max() / np.abs(x[m]).max())
        print('%s: %.3e' % (k, err))
        assert err < 1e-3, k
