"""Fine-tuning rollout without MatterSim (SURVEY §8f N4 + the fine-tuning half of N1).

The reference drives its fine-tuning loop through MatterSim with rendering switched OFF (M/r2r/env.py:47-58): the simulator is
used as a graph walker only — adjacency, headings, the 36 discretised view directions — and everything the model sees is
assembled on the host by Python loops over viewpoint-id strings (M/r2r/agent.py:82-304) around a per-episode `GraphMap`
(M/models/graph_utils.py:43-144) whose incremental Floyd update is an O(N^2) Python double loop per step.

Here (M/ = /root/reference/map_nav_src), one module per layer, each importing only the ones above it in this list:

  * navsim.py       the graph-only navigator and the maps: `ScanGraph` / `GraphSim`, `FloydGraph` / `GraphMap`, `NodeEmbedStore`
                    (the node embeddings, on the device), `ObjectStore` (REVERIE / SOON objects), the angle features.
  * nav_inputs.py   the host input builders `language_inputs`, `panorama_inputs`, `gmap_inputs`, `vp_inputs`, `teacher_action`,
                    `teacher_object`, and the start-of-walk / per-step bookkeeping every walk shares.
  * rollout.py      (this module) `NavRollout`, the eager rollout loop, and the names of all the others: `rollout.<Name>` is the
                    public spelling of every class and function listed here.
  * episodes.py     planned episodes as shape-stable device work: `TeacherEpisode`, `EpisodePlanner`, `PlanWorker`, `EpisodeBuffers`.
  * sampled.py      sampled walks over captured graphs: `SampledEpisode`, `ArgmaxEpisode`, `SinglePassSampledEpisode`.
  * navdev.py       the navigator of those walks on the device: `ScanTables`, `ObjectTables`, `DeviceNavigator` (imports navsim.py, nav_inputs.py).

  * `NavRollout`                  the rollout loop (M/r2r/agent.py:448-676) for feedback = teacher / argmax / sample.  Teacher
                                  forcing needs no device->host copy at all (the next action comes from the ground-truth path), so the
                                  host builds step t+1 while the GPU runs step t; sampled rollouts read back B action indices per
                                  step, as the reference does."""
import time

import numpy as np
import torch

from .navsim import (MAX_DIST, MAX_STEP, FLOYD_INF, HFOV, VFOV, angle_feature, get_angle_fts, view_angles,  # noqa: F401
                     view_angle_feature_table, rel_pos, FloydGraph, GraphMap, NodeEmbedStore, ScanGraph, ObjectStore, GraphSim)
from .nav_inputs import (EXPERT_POLICIES, cal_dtw, language_inputs, panorama_inputs, panorama_object_inputs, gmap_order, gmap_inputs, vp_inputs,  # noqa: F401
                         teacher_object, teacher_action, start_walk, note_step, nodefault, fused_or_mean, pick_logits)
from .episodes import (default_gmap_width, TeacherEpisode, _obj_concat_tables, EpisodePlanner, _RowIndex, _plan_worker_main,  # noqa: F401
                       PlanWorker, _pad1np, EpisodeBuffers)
from .sampled import SampledEpisode, ArgmaxEpisode, SinglePassSampledEpisode  # noqa: F401
from .navdev import ScanTables, ObjectTables, DeviceNavigator  # noqa: F401


# ------------------------------------------------------------------------------------------------ the rollout (agent.py:448-676)
class NavRollout:
    """One rollout of B episodes through a VLNBert-compatible `model(mode, batch)` (nav_model.VLNBert).

        sim = GraphSim(store); ro = NavRollout(model, sim, store, max_action_len=15)
        loss, traj = ro.run(episodes, feedback='teacher', extras={'language': {...BACL/FACL tensors...}, 'panorama': {...}, 'navigation': {...}})

    extras: tensors added verbatim to the input dict of the given mode (the confounder dictionaries z_dicts / z_front_dict of
    M/r2r/agent.py:486-511).  `pano_width` / `gmap_buckets`: pad every step's panorama to a fixed width and the map to the next
    bucket (shape-stable steps: a captured step graph per bucket can be replayed; None = the reference's per-batch maxima)."""

    def __init__(self, model, sim, features, max_action_len=15, fusion='dynamic', ignoreid=-100, pano_width=None, gmap_buckets=None,
                 device='cuda', hoist_text_kv=True, obj_width=None, teacher_scores=True, expert_policy='spl'):
        self.model, self.sim, self.features = model, sim, features
        if expert_policy not in EXPERT_POLICIES:
            raise ValueError('NavRollout: expert_policy is one of %s, got %r' % (EXPERT_POLICIES, expert_policy))
        if expert_policy == 'ndtw' and getattr(sim, 'objects', None) is not None:
            raise ValueError('NavRollout: the REVERIE / SOON agent has the shortest-path expert only; expert_policy=\'ndtw\' needs a walk without objects')
        self.expert_policy = expert_policy      # the DAgger expert of feedback != 'teacher' (M/r2r/agent.py:330-346; 'ndtw' in the RxR scripts)
        self.teacher_scores = teacher_scores    # teacher forcing records stop scores / best objects too, as the reference (one read-back per step)
        self.objects = getattr(sim, 'objects', None)      # REVERIE / SOON: object tokens + object grounding (M/reverie/agent_obj_goat.py:560-790)
        self.obj_width = obj_width
        self.max_action_len, self.fusion, self.ignoreid = max_action_len, fusion, ignoreid
        self.pano_width, self.gmap_buckets = pano_width, gmap_buckets
        self.hoist_text_kv = hoist_text_kv      # K|V projections of the instruction once per episode (nav_model.text_kv) instead of per step
        self.device = torch.device(device)
        self.host_s = 0.0          # seconds spent in the host-side builders during the last run (diagnostics)

    def _bucket(self, n):
        if not self.gmap_buckets:
            return None
        for g in self.gmap_buckets:
            if g >= n:
                return g
        raise ValueError('map with %d nodes exceeds the largest bucket %d' % (n, self.gmap_buckets[-1]))

    def run(self, episodes, feedback='teacher', extras=None, train_ml=1.0, compute_loss=True, sampler=None):
        extras = extras or {}
        dev = self.device
        mv = lambda d: {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in d.items()}
        t_host = time.perf_counter()
        obs, gmaps, traj, store = start_walk(self.sim, episodes)
        B = len(obs)
        if self.objects is not None:
            for tr in traj:
                tr['pred_objid'] = None
        lang = language_inputs(obs)
        self.host_s = time.perf_counter() - t_host
        lang_in = mv(lang)
        lang_in.update(extras.get('language', {}))
        txt_embeds = self.model('language', nodefault(lang_in))
        txt_kv = self.model('text_kv', {'txt_embeds': txt_embeds}) if self.hoist_text_kv else None
        ended = np.zeros(B, bool)
        just_ended = np.zeros(B, bool)
        last_embeds = None
        ml_loss = og_loss = 0.0
        has_obj = self.objects is not None
        steps = 0
        self.actions = []           # the action index of every sample at every step taken (TeacherEpisode.plan(actions=) re-walks them)
        for t in range(self.max_action_len):
            t_host = time.perf_counter()
            pano = panorama_inputs(obs, self.sim.angle_feat_size, self.pano_width, self.obj_width)
            self.host_s += time.perf_counter() - t_host
            pin = {'view_img_fts': self.features.gather(pano['view_rows'].to(dev, non_blocking=True)), 'already_dropout': False}
            pin.update(mv({k: pano[k] for k in ('loc_fts', 'nav_types', 'view_lens')}))
            if has_obj:
                if pano['obj_rows'].shape[1] == 0:          # no viewpoint of this step sees an object: one padding slot (the kernels take no
                    pano['obj_rows'] = torch.full((B, 1), -1, dtype=torch.int64)                # zero-width tensors; obj_lens = 0 masks it)
                    pano['reverie_obj_names'] = torch.zeros((B, 1), dtype=torch.int64)
                    pano['reverie_obj_locs'] = torch.zeros((B, 1, pano['loc_fts'].shape[2]), dtype=torch.float32)
                pin['reverie_obj_img_fts'] = self.objects.gather(pano['obj_rows'].to(dev, non_blocking=True))
                pin.update(mv({k: pano[k] for k in ('reverie_obj_lens', 'reverie_obj_names', 'reverie_obj_locs', 'reverie_obj_nav_types')}))
            pin.update(extras.get('panorama', {}))
            pano_embeds, pano_masks, fused = self.model('panorama', nodefault(pin))
            fused = fused_or_mean(pano_embeds, pano_masks, fused)
            t_host = time.perf_counter()
            store.begin_step(pano_embeds, fused)
            note_step(gmaps, obs, ended, t, store, pano['cand_vpids'])
            n_nodes = max(2 + len(g.node_positions) for g in gmaps)
            gin = gmap_inputs(obs, gmaps, self._bucket(n_nodes), self.sim.angle_feat_size, mem_selectable=has_obj)
            W = pano['nav_types'].shape[1]              # (REVERIE: views + objects)
            vin = vp_inputs(obs, gmaps, pano['cand_vpids'], pano['view_lens'], pano['nav_types'], W + 2, self.sim.angle_feat_size,
                            gmap_pos=(gin['gmap_vpids'], gin['gmap_pos_fts'].numpy()), obj_lens=pano['reverie_obj_lens'] if has_obj else None)
            G = gin['gmap_step_ids'].shape[1]
            nav_vpids = gin['gmap_vpids'] if self.fusion != 'local' else vin['vp_cand_vpids']
            target = None
            if compute_loss or feedback == 'teacher':
                target = teacher_action(obs, nav_vpids, ended, visited_masks=gin['gmap_visited_masks'].numpy() if self.fusion != 'local' else None,
                                        imitation_learning=(feedback == 'teacher' and not has_obj), t=t, ignoreid=self.ignoreid,
                                        expert_policy=self.expert_policy, traj=traj)      # (the REVERIE agent has the shortest-path expert only, M/reverie/agent_obj_goat.py:390-417)
            self.host_s += time.perf_counter() - t_host
            zero = pano_embeds.new_zeros(B, 1, pano_embeds.shape[-1])
            memtok = zero if last_embeds is None else last_embeds.unsqueeze(1).to(pano_embeds.dtype)
            nin = {'txt_embeds': txt_embeds, 'txt_masks': lang_in['txt_masks'],
                   'gmap_img_embeds': store.gather(gin['gmap_vpids'], G, last_embeds),
                   'vp_img_embeds': torch.cat([zero, memtok, pano_embeds], 1), 'vp_obj_masks': None, 'flops_count': False, 'txt_kv': txt_kv}
            nin.update(mv({k: v for k, v in gin.items() if k not in ('gmap_lens', 'no_vp_left')}))
            nin.update(mv(vin))
            nin.update(extras.get('navigation', {}))
            out = self.model('navigation', nodefault(nin))
            last_embeds = out['cls_embeds']
            logits = pick_logits(out, self.fusion)
            steps += 1
            if target is not None and compute_loss:
                ml_loss = ml_loss + torch.nn.functional.cross_entropy(logits.float(), torch.from_numpy(target).to(dev, non_blocking=True),
                                                                      reduction='sum', ignore_index=self.ignoreid)
                if has_obj:                 # object grounding at the goal viewpoints (M/reverie/agent_obj_goat.py:705-707)
                    otgt = teacher_object(obs, ended, pano['view_lens'], self.ignoreid)
                    og_loss = og_loss + torch.nn.functional.cross_entropy(out['obj_logits'].float(), torch.from_numpy(otgt).to(dev, non_blocking=True),
                                                                          reduction='sum', ignore_index=self.ignoreid)
            if feedback not in ('teacher', 'argmax', 'sample'):
                raise ValueError('invalid feedback option %r' % (feedback,))
            if feedback == 'teacher' and not self.teacher_scores:
                a_t = target
                stop = [ob['viewpoint'] == ob['gt_path'][-1] for ob in obs]
            else:
                # ONE device -> host copy per step: the chosen actions and the stop probabilities (M/r2r/agent.py:575-580,601-607).  The
                # reference records the stop score (and the best object) of the current node in EVERY feedback mode
                # (M/reverie/agent_obj_goat.py:679-689,754-761): teacher forcing too, so that its trajectories end with the same stop-node
                # backtrack and predicted object (`teacher_scores=False` skips the read-back where only the loss is used)
                probs = torch.softmax(logits.detach().float(), 1)
                if feedback == 'teacher':
                    act = torch.from_numpy(np.asarray(target, np.int64)).to(probs.device)
                elif feedback == 'argmax':
                    act = probs.argmax(1)
                elif sampler is not None:           # (a fixed action sequence in place of Categorical.sample(): the sampled-rollout golden)
                    act = torch.as_tensor(sampler(t, probs), dtype=torch.int64, device=probs.device)
                else:
                    act = torch.distributions.Categorical(probs).sample()
                rows = [act.to(torch.float32), probs[:, 0].detach()]
                if has_obj:                 # the best object of every sample's current viewpoint rides in the same read-back (:680-690)
                    vl = pano['view_lens'].to(dev)
                    pos = torch.arange(out['obj_logits'].shape[1], device=dev)[None, :]
                    ol = torch.where(pos >= (vl + 2)[:, None], out['obj_logits'].detach().float(), torch.full_like(out['obj_logits'], -float('inf'), dtype=torch.float32))
                    rows.append((ol.argmax(1) - (vl + 2)).to(torch.float32))
                back = torch.stack(rows, 0).cpu().numpy()
                a_t = target if feedback == 'teacher' else back[0].astype(np.int64)
                stop = (a_t == 0) if feedback == 'argmax' else [ob['viewpoint'] == ob['gt_path'][-1] for ob in obs]
                for i, g in enumerate(gmaps):
                    if not ended[i]:
                        g.node_stop_scores[obs[i]['viewpoint']] = {'stop': float(back[1, i])}
                        if has_obj:
                            ids = obs[i]['obj_ids']
                            g.node_stop_scores[obs[i]['viewpoint']]['og'] = ids[int(back[2, i])] if len(ids) > 0 else None
            t_host = time.perf_counter()
            self.actions.append(np.where(ended, 0, np.asarray(a_t, np.int64)))
            moves = []
            for i in range(B):
                forced = bool(stop[i] or ended[i] or gin['no_vp_left'][i] or t == self.max_action_len - 1)
                nxt = None if forced else nav_vpids[i][int(a_t[i])]
                if forced:
                    just_ended[i] = True            # M/r2r/agent.py:657-660: ONLY these four conditions mark the episode for the stop-node backtrack;
                if nxt is None:                     # a sampled action 0 (the [stop] token: nav_vpids[i][0] is None, :661) ends it without one
                    moves.append(None)
                else:
                    hop = gmaps[i].graph.path(obs[i]['viewpoint'], nxt)
                    traj[i]['path'].append(hop)
                    prev = traj[i]['path'][-2][-1] if len(hop) == 1 else hop[-2]
                    view = next(c['pointId'] for c in obs[i]['scan_graph'].candidates(prev) if c['viewpointId'] == nxt)
                    moves.append((nxt, view))
            # go back to the node with the best stop score (M/r2r/agent.py:665-672), in every feedback mode as the reference (with
            # teacher_scores=False a teacher rollout records no scores: its dictionary is empty and nothing moves)
            for i in range(B):
                if (not ended[i]) and just_ended[i] and gmaps[i].node_stop_scores:
                    stop_node, score = max(gmaps[i].node_stop_scores.items(), key=lambda kv: kv[1]['stop'])
                    if obs[i]['viewpoint'] != stop_node:
                        traj[i]['path'].append(gmaps[i].graph.path(obs[i]['viewpoint'], stop_node))
                    if has_obj:
                        traj[i]['pred_objid'] = score.get('og')             # (:761)
            obs = self.sim.step(moves)
            for i, ob in enumerate(obs):
                if not ended[i]:
                    gmaps[i].update_graph(ob)
            ended = np.logical_or(ended, np.array([m is None for m in moves]))
            self.host_s += time.perf_counter() - t_host
            if ended.all():
                break
        loss = ml_loss * train_ml / B if compute_loss else None
        # (the two parts are kept as DETACHED values: an attribute holding a tensor of the autograd graph would keep the graph — and its
        #  AccumulateGrad nodes, bound to this pass's stream — alive past the caller's backward; a later capture of a training step then
        #  accumulates off-graph, see hipops.graph)
        self.ml_loss = loss.detach() if torch.is_tensor(loss) else loss
        self.og_loss = None
        if compute_loss and has_obj:            # self.loss += ml_loss; self.loss += og_loss, both * train_ml / batch_size (:781-787)
            og = og_loss * train_ml / B
            self.og_loss = og.detach()
            loss = loss + og
        self.steps = steps
        return loss, traj
