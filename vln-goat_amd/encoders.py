"""The encoder stems of the pre-training model (pretrain_model.py) and of the navigation model (nav_model.py): language
encoder (plain and BACL / FACL-intervened), panorama embeddings, local and global-map encoder, and the host index tensors the
last two gather through.

The reference keeps two copies of this file (P/model/vilmodel_goat.py:24-527, M/models/vilmodel_GOAT.py:55-510) that drifted
apart: each creates modules the other lacks, and a few sums are written in another order.  Here both trees sit on one definition
per class; what differs is a `_Tree` below, chosen by the constructor's `tree` argument ('pretrain' / 'nav').  The state_dict
keys of either tree (tests/golden/contract_*.json) and the order in which the sub-modules are created — the order of
`named_parameters()` and of the random draws before `init_weights()`, tests/golden/module_tree_order.json — are as in the
reference's copy for that tree.
"""
from typing import Callable, NamedTuple

import torch
from torch import nn

from . import graphmap, hipops
from .layers import (BertAttention, BertLayerNorm, CrossmodalEncoder, Linear, RobertaLayer, _p, compute_dtype,
                     create_transformer_encoder, gen_seq_masks)


class _Tree(NamedTuple):
    # LanguageEncoderDo
    z_cross_attn: bool          # type_1 under config.z_cross_attn: the dictionaries attend to the text first (modules + step)
    txt_self_attn: bool         # created under type_2, never used (checkpoint compat)
    cast_dicts: bool            # dictionaries are cast to the compute dtype on entry; False: type_1 sums them as they come (float32)
    # CausalImageEmbeddings
    img_self_attn: bool         # created, never used (checkpoint compat)
    back_img: bool              # BACL-img modules and intervene(); False: config.do_back_img is refused
    obj_name_always: bool       # obj_name_linear exists regardless of config.use_obj_name
    nav_type_first: bool        # REVERIE tokens: x + nav_type + loc; False: x + loc + nav_type (another rounding in bf16)
    # LocalVPEncoder / GlobalMapEncoder
    lang_branch: bool           # CrossmodalEncoder(with_lang_branch=)
    tim: Callable               # config -> the CFP self-attention block (tim_self_encoder) exists
    sprel_last: bool            # GlobalMapEncoder creates sprel_linear after tim_self_encoder; False: before


TREES = {
    # (do_back_img: the upstream BACL-img pretrain branch is broken, SURVEY §8a-Q viii)
    'pretrain': _Tree(z_cross_attn=True, txt_self_attn=True, cast_dicts=True, img_self_attn=True, back_img=False, obj_name_always=True,
                      nav_type_first=True, lang_branch=True, tim=lambda c: 'cfp' in c.pretrain_tasks, sprel_last=True),
    'nav': _Tree(z_cross_attn=False, txt_self_attn=False, cast_dicts=False, img_self_attn=False, back_img=True, obj_name_always=False,
                 nav_type_first=False, lang_branch=False, tim=lambda c: c.mode == 'extract_cfp_features', sprel_last=False),
}


def _door(aug_lin, ori_lin, aug, ori):
    """door gate: w = sigmoid(Linear_a(aug) + Linear_o(ori)); out = w*aug + (1-w)*ori
    (P/model/vilmodel_goat.py:137-143; M/models/vilmodel_GOAT.py:147-153, 548-552)."""
    return hipops.door_gate(aug_lin, ori_lin, aug, ori)


class LanguageEncoder(nn.Module):
    # P/model/vilmodel_goat.py:24-44
    def __init__(self, config):
        super().__init__()
        self.num_l_layers = config.num_l_layers
        self.update_lang_bert = config.update_lang_bert
        self.layer = nn.ModuleList([RobertaLayer(config) for _ in range(self.num_l_layers)])
        if not self.update_lang_bert:
            for _, param in self.layer.named_parameters():
                param.requires_grad = False

    def forward(self, txt_embeds, txt_kmask, *unused):
        """txt_kmask: additive key mask (layers.neg_mask of the token mask)."""
        for i, layer in enumerate(self.layer):       # between layers the state travels as a layers._pair (fork=True)
            txt_embeds = layer(txt_embeds, txt_kmask, fork=i + 1 < len(self.layer))
        if not self.update_lang_bert:
            txt_embeds = txt_embeds.detach()
        return txt_embeds


class LanguageEncoderDo(LanguageEncoder):
    """BACL-txt / FACL-txt (P/model/vilmodel_goat.py:46-159, M/models/vilmodel_GOAT.py:55-162): after the RoBERTa layers the text
    is intervened with the direction / landmark confounder dictionaries — type_1: probability-weighted dictionary sums through
    three Linears (pre-training: optionally dictionary->text cross-attention first, z_cross_attn); type_2: text->dictionary
    cross-attention, then door / add / concat — and with the front-door text features (navigation; the pre-training tree creates
    z_front_* and never passes any), followed by LayerNorm.  The module set mirrors the reference's constructor of either tree."""

    def __init__(self, config, tree):
        super().__init__(config)
        self.config = config
        self.tree = TREES[tree]
        H = config.hidden_size
        front = getattr(config, 'do_front_txt', False)
        if config.do_back_txt or front:         # (the pre-training model builds this class under do_back_txt only)
            if self.tree.z_cross_attn and config.z_cross_attn:
                self.z_direc_cross_attn = BertAttention(config)
                self.z_landm_cross_attn = BertAttention(config)
            self.z_txt_linear = Linear(H, H)
            self.z_direct_linear = Linear(H, H)
            self.z_landm_linear = Linear(H, H)
            self.z_concat_layernorm = BertLayerNorm(H, eps=config.layer_norm_eps)
            self.z_direct_ln = BertLayerNorm(H, eps=config.layer_norm_eps)
            self.z_landm_ln = BertLayerNorm(H, eps=config.layer_norm_eps)
            if config.do_back_txt_type == 'type_2':
                # (with z_cross_attn on as well these two are built a second time, as in the reference: the first pair keeps its
                #  place in the module order and its random draws, the second pair is the one that stays)
                self.z_direc_cross_attn = BertAttention(config)
                self.z_landm_cross_attn = BertAttention(config)
                if self.tree.txt_self_attn:
                    self.txt_self_attn = BertAttention(config)
                self.instr_aug_linear = Linear(H, 1)
                self.instr_ori_linear = Linear(H, 1)
                self.instr_sigmoid = nn.Sigmoid()
                self.concat_linear = Linear(H * 3, H)
        if front:
            self.z_front_cross_attn = BertAttention(config)
            self.z_front_linear = Linear(H, H)
            self.z_front_ln = BertLayerNorm(H, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, txt_embeds, txt_kmask, z_direc=None, z_direc_pzs=None, z_landm=None, z_landm_pzs=None, front_txt=None):
        cfg = self.config
        txt_embeds = super().forward(txt_embeds, txt_kmask)
        if cfg.do_back_txt and z_direc is None:          # no dictionaries: the plain text states
            return txt_embeds
        dt = txt_embeds.dtype
        front = front_txt is not None and getattr(cfg, 'do_front_txt', False)
        if self.tree.cast_dicts and z_direc is not None:
            z_direc, z_landm = z_direc.to(dt), (z_landm.to(dt) if z_landm is not None else None)
        if cfg.do_back_txt_type == 'type_1':
            if cfg.do_back_txt:
                if self.tree.z_cross_attn and cfg.z_cross_attn:       # dictionary entries attend to the (key-masked) text
                    z_direc = self.z_direc_cross_attn(z_direc, None, txt_embeds, txt_kmask)
                    z_landm = self.z_landm_cross_attn(z_landm, None, txt_embeds, txt_kmask)
                sd = hipops.dict_weighted_sum(z_direc, z_direc_pzs, dt)
                sl = hipops.dict_weighted_sum(z_landm, z_landm_pzs, dt)
                txt_embeds = self.z_txt_linear(txt_embeds) + self.z_direct_linear(sd) + self.z_landm_linear(sl)
            if front:
                zf = self.z_front_cross_attn(txt_embeds, None, front_txt.to(dt), None)
                txt_embeds = txt_embeds + self.z_front_ln(self.z_front_linear(zf))
            return self.z_concat_layernorm(txt_embeds)
        # type_2: the text attends to each dictionary (no key mask on dictionary entries)
        zd = zl = z_front = None
        if cfg.do_back_txt:
            zd = self.z_direct_ln(self.z_direct_linear(self.z_direc_cross_attn(txt_embeds, None, z_direc.to(dt), None)))
            if z_landm is not None:
                zl = self.z_landm_ln(self.z_landm_linear(self.z_landm_cross_attn(txt_embeds, None, z_landm.to(dt), None)))
        if front:
            z_front = self.z_front_ln(self.z_front_linear(self.z_front_cross_attn(txt_embeds, None, front_txt.to(dt), None)))
        if cfg.do_add_method == 'door':
            aug = zd
            if zl is not None:
                aug = aug + zl
            if z_front is not None:
                aug = z_front if aug is None else aug + z_front
            txt_embeds = _door(self.instr_aug_linear, self.instr_ori_linear, aug, txt_embeds)
        elif cfg.do_add_method == 'add':
            if cfg.do_back_txt:
                txt_embeds = txt_embeds + zd + zl
            if front:
                txt_embeds = txt_embeds + z_front
        elif cfg.do_add_method == 'concat':
            txt_embeds = self.concat_linear(torch.cat((txt_embeds, zd, zl), -1))
        return self.z_concat_layernorm(txt_embeds)


class CausalImageEmbeddings(nn.Module):
    """P/model/vilmodel_goat.py:234-364, M/models/vilmodel_GOAT.py:164-316: the R2R / RxR branch (view + location embeddings
    through the panorama encoder) and the REVERIE / SOON branch (object tokens appended to every panorama, P:322-349, M:693-720),
    with the BACL-img intervention in the navigation tree."""

    def __init__(self, config, tree):
        super().__init__()
        self.config = config
        self.tree = TREES[tree]
        self.reverie = getattr(config, 'name', 'R2R') in ('REVERIE', 'SOON')
        self.do_back_img = getattr(config, 'do_back_img', False)
        if self.do_back_img and not self.tree.back_img:
            raise NotImplementedError('pretrain do_back_img is broken upstream (undefined do_back_img_after_linear)')
        H = config.hidden_size
        self.img_linear = Linear(config.image_feat_size, H)
        self.img_layer_norm = BertLayerNorm(H, eps=1e-12)
        self.loc_linear = Linear(config.angle_feat_size + 3, H)
        self.loc_layer_norm = BertLayerNorm(H, eps=1e-12)
        if not self.reverie:
            if self.tree.img_self_attn:
                self.img_self_attn = BertAttention(config)
            self.img_self_encoder = create_transformer_encoder(config, config.num_pano_layers, norm=True)
        if self.do_back_img:
            self.do_img_before_linear = Linear(config.image_feat_size, H)
            self.do_img_layer_norm = BertLayerNorm(H, eps=1e-12)
            self.do_img_attn = BertAttention(config)
            self.do_img_after_linear = Linear(H, H)
            self.img_after_linear = Linear(H, H)
            self.do_img_concat_layernorm = BertLayerNorm(H, eps=1e-12)
            if config.do_back_img_type == 'type_2':
                if config.do_add_method == 'door':
                    self.sigmoid = nn.Sigmoid()
                elif config.do_add_method == 'concat':
                    self.do_concat_img_linear = Linear(H * 2, H)
        if self.reverie:
            if self.tree.obj_name_always or config.use_obj_name:
                self.obj_name_linear = nn.Embedding(config.obj_name_vocab_size, H)
            self.obj_reverie_linear = Linear(config.obj_feat_size, H)
            self.obj_reverie_layer_norm = BertLayerNorm(H, eps=1e-12)
            self.nav_type_embedding = nn.Embedding(3, H)
            self.pano_encoder = create_transformer_encoder(config, config.num_pano_layers, norm=True)
        else:
            self.nav_type_embedding = nn.Embedding(2, H)    # unused on R2R
        if config.adaptive_pano_fusion:
            self.adaptive_pano_attn = Linear(H, 1)
        self.layer_norm = BertLayerNorm(H, eps=1e-12)       # unused on R2R
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def intervene(self, x, z_img_features, z_img_pzs):
        """BACL-img (M/models/vilmodel_GOAT.py:659-681)."""
        cfg = self.config
        dt = x.dtype
        z = self.do_img_layer_norm(self.do_img_before_linear(z_img_features.to(dt)))
        if cfg.do_back_img_type == 'type_1':
            s = hipops.dict_weighted_sum(z, z_img_pzs, dt)
            x = self.img_after_linear(x) + self.do_img_after_linear(s)
        else:
            z = self.do_img_attn(x, None, z, None)
            if cfg.do_add_method == 'door':
                w = torch.sigmoid(self.img_after_linear(x).float() + self.do_img_after_linear(z).float()).to(dt)
                x = w * x + (1 - w) * z
            elif cfg.do_add_method == 'add':
                x = x + z
            elif cfg.do_add_method == 'concat':
                x = self.do_concat_img_linear(torch.cat((x, z), -1))
        return self.do_img_concat_layernorm(x)

    def encode(self, view_img_fts, loc_fts, view_lens, z_img_features=None, z_img_pzs=None, loc_before=False,
               nav_types=None, obj_fts=None, obj_lens=None, obj_names=None, obj_concat=None):
        """-> (embeds [N,W,H], masks [N,W] bool, fused [N,H] | None).  `loc_before`: the location is added before the intervention
        (M:225-252, the CFP feature extraction); pre-training and per-step navigation add it after (M:688-691).
        REVERIE/SOON: object tokens follow the views of every row; loc_fts / nav_types are [N,W,...]; obj_concat =
        graphmap.build_obj_concat_index(...) on the device, optionally followed by its graphmap.inverse_index."""
        dt = compute_dtype()
        x = self.img_layer_norm(self.img_linear(view_img_fts.to(dt)))
        if self.reverie:
            if z_img_features is not None:
                x = self.intervene(x, z_img_features, z_img_pzs)
            o = self.obj_reverie_linear(obj_fts.to(dt))
            if self.config.use_obj_name:
                o = o + hipops.embedding(obj_names, self.obj_name_linear.weight, out_dtype=dt)
            o = self.obj_reverie_layer_norm(o)
            N, V, H = x.shape
            W = nav_types.shape[1]
            src = torch.cat([x.reshape(N * V, H), o.reshape(-1, H)], 0)
            if obj_concat is not None:      # already on the device: shape-stable callers (captured steps and episodes: no host read of the lengths)
                x = hipops.gather_segmean(src, obj_concat[0], obj_concat[1], None, N * W, tuple(obj_concat[2:4]) or None).view(N, W, H)
            else:
                ci = graphmap.build_obj_concat_index(view_lens, obj_lens, V, o.shape[1], W)
                x = hipops.gather_segmean(src, ci[0].to(x.device), ci[1].to(x.device), None, N * W).view(N, W, H)
            # (the two trees add the same three terms in another order: kept, the sums round differently in bf16)
            if self.tree.nav_type_first:
                x = x + hipops.embedding(nav_types, self.nav_type_embedding.weight, out_dtype=dt) \
                    + self.loc_layer_norm(self.loc_linear(loc_fts.to(dt)))
            else:
                x = x + self.loc_layer_norm(self.loc_linear(loc_fts.to(dt))) \
                    + hipops.embedding(nav_types, self.nav_type_embedding.weight, out_dtype=dt)
            x = self.layer_norm(x, p_out=_p(self.dropout))
            masks = gen_seq_masks(view_lens + obj_lens, W)
            x = self.pano_encoder(x, masks)
        else:
            loc_in = self.loc_linear(loc_fts.to(dt))
            if loc_before:
                x = x + self.loc_layer_norm(loc_in)
            if z_img_features is not None:
                x = self.intervene(x, z_img_features, z_img_pzs)
            if not loc_before:       # dropout(x + loc_LN(...)): the sum and the dropout inside the LayerNorm's launch
                x = self.loc_layer_norm(loc_in, post_add=x, p_out=_p(self.dropout))
            else:
                x = hipops.dropout(x, _p(self.dropout))
            masks = gen_seq_masks(view_lens, view_img_fts.shape[1])
            x = self.img_self_encoder(x, masks)
        fused = None
        if self.config.adaptive_pano_fusion:
            fused = hipops.pano_fusion(x, self.adaptive_pano_attn.weight, self.adaptive_pano_attn.bias)
        return x, masks, fused

    def forward(self, traj_view_img_fts, traj_loc_fts, traj_vp_view_lens, traj_nav_types=None, obj_fts=None, obj_lens=None,
                obj_names=None, cat_index=None, cat_inverse=None):
        """The pre-training entry (a whole trajectory batch, indices from the batch cache) -> (tokens [N,W,H], fused [N,H] | None).
        cat_index = graphmap.build_obj_concat_index(...) on device (cat_inverse: its graphmap.inverse_index, optional)."""
        obj_concat = None if cat_index is None else tuple(cat_index) + tuple(cat_inverse or ())
        x, _, fused = self.encode(traj_view_img_fts, traj_loc_fts, traj_vp_view_lens, nav_types=traj_nav_types, obj_fts=obj_fts,
                                  obj_lens=obj_lens, obj_names=obj_names, obj_concat=obj_concat)
        return x, fused


class LocalVPEncoder(nn.Module):
    # P/model/vilmodel_goat.py:366-410
    def __init__(self, config, tree):
        super().__init__()
        tree = TREES[tree]
        self.vp_pos_embeddings = nn.Sequential(Linear(config.angle_feat_size * 2 + 6, config.hidden_size),
                                               BertLayerNorm(config.hidden_size, eps=1e-12))
        self.encoder = CrossmodalEncoder(config, with_lang_branch=tree.lang_branch)
        if tree.tim(config):
            self.tim_self_encoder = BertAttention(config)

    def vp_input_embedding(self, pano_embeds, idx, vp_pos_fts, inverse=None):
        """pano_embeds [N,V,H]; idx = graphmap.build_vp_index(...) on device (inverse: its graphmap.inverse_index, optional)."""
        vidx, vstart, vp_lens, width = idx
        B = vp_pos_fts.shape[0]
        vp_img = hipops.gather_segmean(pano_embeds, vidx, vstart, None, B * width, inverse).view(B, width, -1)
        # (kept as a separate add: folding it into the LayerNorm launch (post_add) removes one bf16 rounding, which moved the most
        #  noise-sensitive gradient of the model — sap_fuse_linear, a difference of two softmax-weighted sums — past its calibrated
        #  bf16 bound in 2 of 16 parity cases; 3 us per step are not worth re-calibrating the bound)
        pos = self.vp_pos_embeddings[1](self.vp_pos_embeddings[0](vp_pos_fts[:, :width].to(vp_img.dtype)))
        return vp_img + pos, gen_seq_masks(vp_lens, width)


class GlobalMapEncoder(nn.Module):
    # P/model/vilmodel_goat.py:412-527
    def __init__(self, config, tree):
        super().__init__()
        tree = TREES[tree]
        self.gmap_pos_embeddings = nn.Sequential(Linear(config.angle_feat_size + 3, config.hidden_size),
                                                 BertLayerNorm(config.hidden_size, eps=1e-12))
        self.gmap_step_embeddings = nn.Embedding(config.max_action_steps, config.hidden_size)
        self.encoder = CrossmodalEncoder(config, with_lang_branch=tree.lang_branch)
        if not tree.sprel_last:
            self.sprel_linear = Linear(1, 1) if config.graph_sprels else None
        if tree.tim(config):
            self.tim_self_encoder = BertAttention(config)
        if tree.sprel_last:
            self.sprel_linear = Linear(1, 1) if config.graph_sprels else None

    def gmap_input_embedding(self, src_rows, idx, gmap_step_ids, gmap_pos_fts, gmap_lens, inverse=None):
        """src_rows: panorama tokens [N*V,H] (+ fused rows [N,H]); idx = graphmap.build_gmap_index(...) on device."""
        gidx, gstart, gscale = idx
        B, G = gmap_step_ids.shape
        img = hipops.gather_segmean(src_rows, gidx, gstart, gscale, B * G, inverse).view(B, G, -1)
        pos = self.gmap_pos_embeddings[1](self.gmap_pos_embeddings[0](gmap_pos_fts.to(img.dtype)))
        e = img + hipops.embedding(gmap_step_ids, self.gmap_step_embeddings.weight, out_dtype=img.dtype) + pos
        return e, gen_seq_masks(gmap_lens, G)

    def sprels(self, gmap_pair_dists):
        # Linear(1,1) on the distance matrix (:496-497); float32, gradient flows back through the attention bias
        w, b = self.sprel_linear.weight.view(()), self.sprel_linear.bias.view(())
        return gmap_pair_dists.float() * w + b


def trajectory_indices(batch, fused, inverse=True):
    """Index tensors of a trajectory batch for CausalImageEmbeddings.forward ('objcat'), gmap_input_embedding ('gmap') and
    vp_input_embedding ('vp'), on the device of the batch.  fused: the batch's panoramas carry a fused row each
    (adaptive_pano_fusion).  inverse: also the inverse indices ('*_inv'), with which the backward passes of the gathers are
    gathers over the output gradients (no atomics / fills)."""
    dev = batch['traj_view_img_fts'].device
    V = batch['traj_view_img_fts'].shape[1]
    G = batch['gmap_step_ids'].shape[1]
    lens_cpu = batch['traj_vp_view_lens'].cpu()
    n_rows = int(lens_cpu.shape[0])
    out = {}
    if batch.get('traj_obj_img_fts') is not None:
        # REVERIE/SOON: every panorama row becomes [views | objects], W slots wide (P/model/vilmodel_goat.py:331-341)
        obj_cpu = batch['traj_vp_obj_lens'].cpu()
        O, W = batch['traj_obj_img_fts'].shape[1], batch['traj_nav_types'].shape[1]
        ci = graphmap.build_obj_concat_index(lens_cpu, obj_cpu, V, O, W)
        out['objcat'] = (ci[0].to(dev), ci[1].to(dev))
        if inverse:
            out['objcat_inv'] = tuple(t.to(dev) for t in graphmap.inverse_index(ci[0], ci[1], None, n_rows * V + n_rows * O) if t is not None)
        out['view_lens_cpu'], out['obj_lens_cpu'] = lens_cpu, obj_cpu
        lens_cpu, V = lens_cpu + obj_cpu, W
    g = graphmap.build_gmap_index(batch['traj_step_lens'], lens_cpu, batch['traj_vpids'],
                                  batch['traj_cand_vpids'], batch['gmap_vpids'], G, V, fused)
    v = graphmap.build_vp_index(batch['traj_step_lens'], lens_cpu, V)
    out['gmap'] = tuple(t.to(dev) for t in g)
    out['vp'] = (v[0].to(dev), v[1].to(dev), v[2].to(dev), v[3])
    if inverse:
        out['gmap_inv'] = tuple(t.to(dev) for t in graphmap.inverse_index(g[0], g[1], g[2], n_rows * V + (n_rows if fused else 0)))
        out['vp_inv'] = tuple(t.to(dev) for t in graphmap.inverse_index(v[0], v[1], None, n_rows * V) if t is not None)
    return out
