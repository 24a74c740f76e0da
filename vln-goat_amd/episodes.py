"""Planned episodes of the fine-tuning rollout as shape-stable device work (overview: rollout.py).  Built on navsim.py and
nav_inputs.py; never imports rollout.py, and `nav_model` / `graphmap` only inside the functions that need them: the worker process
of `PlanWorker` imports this module, builds plans on the host and never initialises the GPU.

  * `TeacherEpisode`              a teacher-forced rollout (M/r2r/agent.py:414-420,592-594): `plan()` builds the host tables of all
                                  steps, `body()` is pure device code over them, captured once into a hipGraph and replayed.
  * `EpisodePlanner`              `plan()` one step at a time (a sampled walk decides each move from the step's logits).
  * `PlanWorker`                  `plan()` in a worker process beside the training process.
  * `EpisodeBuffers`              the tensors of a plan at fixed device addresses, fed by one pinned H2D copy."""
import multiprocessing as mp
import os
import queue
import threading
import time

import numpy as np
import torch

from . import hipops, layers
from .navsim import GraphSim
from .nav_inputs import (EXPERT_POLICIES, language_inputs, panorama_inputs, gmap_inputs, vp_inputs, teacher_object, teacher_action,
                         start_walk, note_step, nodefault, fused_or_mean, pick_logits)


# ------------------------------------------------------------------------------------------------ teacher-forced episodes as ONE graph
def default_gmap_width(t, max_degree=7, granule=16):
    """map bucket of step t: [stop], [MEM], t + 1 visited nodes and at most max_degree fresh candidates per visit, rounded up."""
    n = 2 + (t + 1) * (1 + max_degree)
    return (n + granule - 1) // granule * granule


class TeacherEpisode:
    """A teacher-forced rollout (imitation learning, feedback = 'teacher': M/r2r/agent.py:414-420,592-594) as shape-stable device
    work.  With teacher forcing nothing the host builds depends on a model output: the walk follows the ground-truth paths, so the
    maps, positions, masks, logit-fusion matrices, targets and the gather indices of the node embeddings of ALL steps are known
    before the first kernel runs.  `plan()` builds them (numpy, fixed shapes: text bucket L, panorama width W, map width per
    step), `EpisodeBuffers` holds them in one device buffer fed by one pinned H2D copy, and `body()` is pure device code over
    those tensors — captured once into a hipGraph, it is replayed for every new batch of episodes.  Episodes shorter than the
    plan's step count carry target -100 (ignored) after their end, as the reference's `ended` bookkeeping does."""

    def __init__(self, sim, features, n_steps, text_len, pano_width=40, gmap_width=default_gmap_width, fusion='dynamic', ignoreid=-100,
                 obj_width=20, expert_policy='spl'):
        self.sim, self.features = sim, features
        self.T, self.L, self.W, self.gw = n_steps, text_len, pano_width, gmap_width
        self.fusion, self.ignoreid = fusion, ignoreid
        # REVERIE / SOON (sim.objects: an ObjectStore): up to `obj_width` object tokens behind the views of every panorama, the
        # object-grounding loss at goal viewpoints (M/reverie/agent_obj_goat.py:560-790).  WT = tokens per panorama (views + objects).
        self.objects = getattr(sim, 'objects', None)
        self.O = obj_width if self.objects is not None else 0
        self.WT = self.W + self.O
        # the DAgger expert of the states a sampled walk visits (plan(actions=), EpisodePlanner(imitation=False)): 'spl', or 'ndtw' as the
        # RxR scripts set it (M/r2r/agent.py:330-346).  The REVERIE agent has the shortest-path expert only (M/reverie/agent_obj_goat.py:390-417).
        if expert_policy not in EXPERT_POLICIES:
            raise ValueError('TeacherEpisode: expert_policy is one of %s, got %r' % (EXPERT_POLICIES, expert_policy))
        if expert_policy == 'ndtw' and self.objects is not None:
            raise ValueError('TeacherEpisode: the REVERIE / SOON agent has the shortest-path expert only; expert_policy=\'ndtw\' needs a walk without objects')
        self.expert_policy = expert_policy

    # ---- host ---------------------------------------------------------------------------------------------------------------
    def plan(self, episodes, actions=None):
        """host tables of all T steps.  actions=None: the teacher-forced walk along the ground-truth paths (imitation labels).
        actions = [steps, B] action indices into the step's map nodes (0 = [stop]), e.g. NavRollout.actions of a sampled rollout run
        under no_grad: the walk follows THEM — the policy's own path — and the targets are the DAgger labels of the states it visits
        (`teacher_action(imitation_learning=False)`: M/r2r/agent.py:325-347), the episode ends as the sampled rollout does
        (:601-607,657-663: at the goal, on a sampled [stop], with no node left, at the last step).  One replay of the captured body then
        gives the loss and the gradients of the sampled half of the dagger iteration (:436-437) without an eager autograd pass."""
        if actions is not None:
            actions = [np.asarray(a, np.int64) for a in actions]
            if len(actions) > self.T:
                raise ValueError('%d recorded steps exceed the episode bucket T = %d' % (len(actions), self.T))
            if any(a.shape != (len(episodes),) for a in actions):
                raise ValueError('actions must hold one index per episode and step')
        p = EpisodePlanner(self, episodes, imitation=actions is None)
        for t in range(self.T):
            p.build_step()
            p.advance(None if actions is None else (actions[t] if t < len(actions) else np.zeros(len(episodes), np.int64)))
        return p.finish()

    # ---- device -------------------------------------------------------------------------------------------------------------
    def _panoramas(self, model, t_, extras, k, n, B):
        """panorama encoder over the n panoramas of the tables with prefix k ('s<t>_': B of one step, 'all_': T * B)."""
        fts = hipops.gather_segmean(self.features.dev, t_[k + 'feat_idx'], t_[k + 'feat_start'], None, n * self.W, None)
        pin = {'view_img_fts': fts.view(n, self.W, -1), 'loc_fts': t_[k + 'loc_fts'], 'nav_types': t_[k + 'nav_types'],
               'view_lens': t_[k + 'view_lens'], 'already_dropout': False}
        if self.objects is not None:
            ofts = hipops.gather_segmean(self.objects._fs.dev, t_[k + 'obj_idx'], t_[k + 'obj_start'], None, n * self.O, None)
            pin.update({'reverie_obj_img_fts': ofts.view(n, self.O, -1), 'reverie_obj_lens': t_[k + 'reverie_obj_lens'],
                        'reverie_obj_names': t_[k + 'reverie_obj_names'],
                        'reverie_obj_concat': (t_[k + 'ocat_idx'], t_[k + 'ocat_start'], t_[k + 'ocat_inv_idx'], t_[k + 'ocat_inv_start'])})
        for name, z in (extras or {}).get('panorama', {}).items():      # per-sample dictionary copies ([B, K, ...]) follow the joint batch
            pin[name] = z.repeat(n // B, *([1] * (z.dim() - 1))) if (torch.is_tensor(z) and n != B and z.dim() > 1 and z.shape[0] == B) else z
        return model('panorama', nodefault(pin))

    @staticmethod
    def _nav_extras(extras, dtype):
        nav_extras = dict((extras or {}).get('navigation', {}))
        for name in ('front_vp_feats', 'front_gmap_feats', 'front_txt_feats'):      # constant over the episode: cast once, not per step
            if torch.is_tensor(nav_extras.get(name)) and nav_extras[name].is_floating_point():
                nav_extras[name] = nav_extras[name].to(dtype)
        return nav_extras

    def _nav_step(self, model, t_, s, txt, txt_kv, pano, pmask, fused, pool, last, nav_extras):
        """navigation step s over the tables 's<s>_*': node embeddings gathered from `pool` (the panoramas of this and all earlier steps,
        appended to here) and the previous [MEM] state `last`.  -> (logits of the configured fusion, the new [MEM] state, object logits | None)"""
        k = 's%d_' % s
        B = pano.shape[0]
        fused = fused_or_mean(pano, pmask, fused)
        H = pano.shape[-1]
        pool += [pano.reshape(B * self.WT, H), fused.to(pano.dtype)]
        src = torch.cat(pool + ([last.to(pano.dtype)] if last is not None else []), 0)
        G = t_[k + 'gmap_step_ids'].shape[1]
        gimg = hipops.gather_segmean(src, t_[k + 'csr_idx'], t_[k + 'csr_start'], t_[k + 'csr_scale'], B * G,
                                     (t_[k + 'inv_idx'], t_[k + 'inv_start'], t_[k + 'inv_w'])).view(B, G, H)
        zero = pano.new_zeros(B, 1, H)
        memtok = zero if last is None else last.unsqueeze(1).to(pano.dtype)
        nin = {'txt_embeds': txt, 'txt_masks': t_['txt_masks'], 'gmap_img_embeds': gimg,
               'vp_img_embeds': torch.cat([zero, memtok, pano], 1), 'flops_count': False, 'txt_kv': txt_kv,
               'vp_obj_masks': t_[k + 'vp_obj_masks'] if self.objects is not None else None, 'nav_fusion': t_[k + 'nav_fusion']}
        for name in ('gmap_step_ids', 'gmap_pos_fts', 'gmap_pair_dists', 'gmap_visited_masks', 'gmap_masks', 'vp_pos_fts', 'vp_masks',
                     'vp_nav_masks'):
            nin[name] = t_[k + name]
        nin.update(nav_extras)
        out = model('navigation', nodefault(nin))
        logits = pick_logits(out, self.fusion)
        # (the object logits are RETURNED, not kept on self: a tensor of a warm-up pass alive at capture time keeps that pass's autograd
        #  graph alive, whose AccumulateGrad nodes are bound to the warm-up stream — the captured backward then accumulates off-graph)
        return logits, out['cls_embeds'], out.get('obj_logits')

    def _instruction(self, model, t_, extras, handles, hoist_text_kv=True):
        """the instruction pass over the text tables -> (txt, txt_kv | None).  handles: the pass is differentiated — one autograd
        handle per step on the instruction states and their hoisted K|V projections (hipops.fanout) -> (txt_h [T + 1], kv_h [T])."""
        lang = {'txt_ids': t_['txt_ids'], 'txt_masks': t_['txt_masks']}
        lang.update(extras.get('language', {}))
        txt = model('language', nodefault(lang))
        if not handles:
            return txt, (model('text_kv', {'txt_embeds': txt}) if hoist_text_kv else None)
        txt_h = hipops.fanout(txt, self.T + 1)
        txt_kv = model('text_kv', {'txt_embeds': txt_h[self.T]}) if hoist_text_kv else None
        return txt_h, (hipops.fanout_tree(txt_kv, self.T) if txt_kv is not None else [None] * self.T)

    def _loss_rows(self, t_, s, logits, obj_logits):
        """cross-entropy rows of step s: actions and, with objects, object grounding at the goals (M/reverie/agent_obj_goat.py:705-707)"""
        k = 's%d_' % s
        rows = [hipops.cross_entropy_rows(logits, t_[k + 'target'], self.ignoreid)]
        if self.objects is not None:
            rows.append(hipops.cross_entropy_rows(obj_logits, t_[k + 'obj_target'], self.ignoreid))
        return rows

    def body(self, model, bufs, extras=None, hoist_text_kv=True, hoist_pano=True):
        """forward + imitation loss of the planned episodes from the tensors of `bufs` (EpisodeBuffers.t): no host data, no
        device -> host copy.  -> loss (sum over steps and samples of the cross-entropy / B, M/r2r/agent.py:664-667).
        hoist_pano: ONE panorama-encoder call over the T * B panoramas of the whole walk instead of one per step — the encoder sees
        the observation only (M/r2r/agent.py:548-556), and with teacher forcing every observation is known before the first step, so
        its T small launches-bound passes (B * W = 456 rows at B = 12) become one of T * B * W rows; the [MEM]-carrying navigation
        steps stay sequential.  Same embeddings and gradients (summation order aside; dropout draws differ)."""
        extras = extras or {}
        t_ = bufs.t
        B = t_['txt_ids'].shape[0]
        pool, last, loss, ce_rows = [], None, 0.0, []
        panoramas = lambda k, n: self._panoramas(model, t_, extras, k, n, B)

        # (the hoisted panorama pass depends on the observations only: a parallel branch of the instruction encoder in the captured graph)
        with hipops.Branch('pano', 'nav_pano') as bp:
            whole = panoramas('all_', self.T * B) if hoist_pano else None
        txt_h, kv_h = self._instruction(model, t_, extras, True, hoist_text_kv)
        if whole is not None:
            bp.join(*whole)
            # (unbind: ONE backward node stacks the per-step gradients — not T zero-filled slice_backward tensors and T - 1 adds)
            whole_s = [None if x is None else x.view(self.T, B, *x.shape[1:]).unbind(0) for x in whole]
        nav_extras = self._nav_extras(extras, txt_h[0].dtype)
        for s in range(self.T):
            k = 's%d_' % s
            if whole is not None:
                pano, pmask, fused = (None if x is None else x[s] for x in whole_s)
            else:
                pano, pmask, fused = panoramas(k, B)
            logits, last, obj_logits = self._nav_step(model, t_, s, txt_h[s], kv_h[s], pano, pmask, fused, pool, last, nav_extras)
            if self.ignoreid < 0:
                ce_rows += self._loss_rows(t_, s, logits, obj_logits)          # (summed once behind the loop)
            else:
                loss = loss + torch.nn.functional.cross_entropy(logits.float(), t_[k + 'target'], reduction='sum', ignore_index=self.ignoreid)
                if self.objects is not None:
                    loss = loss + torch.nn.functional.cross_entropy(obj_logits.float(), t_[k + 'obj_target'], reduction='sum', ignore_index=self.ignoreid)
        if ce_rows:
            loss = loss + torch.stack(ce_rows, 0).sum()
        return loss / B


def _obj_concat_tables(view_lens, obj_lens, V, O, W, prefix):
    """the [views | objects] row assembly of n panoramas (graphmap.build_obj_concat_index) and its inverse as fixed-size tables"""
    from . import graphmap        # (lazy: as in EpisodePlanner.build_step)
    n = len(view_lens)
    ci = graphmap.build_obj_concat_index(view_lens, obj_lens, V, O, W)
    inv = graphmap.inverse_index(ci[0], ci[1], None, n * V + n * O)
    n_tok = int(ci[1][-1])
    return {prefix + 'ocat_idx': _pad1np(ci[0].numpy()[:n_tok], n * W, -1, np.int32), prefix + 'ocat_start': ci[1],
            prefix + 'ocat_inv_idx': _pad1np(inv[0].numpy()[:n_tok], n * W, -1, np.int32), prefix + 'ocat_inv_start': inv[1]}


def _compact_rows(rows):
    """compact CSR of a gather over `rows` [n, w] (-1: padding) -> (idx [n * w]: the valid rows, then -1; start [n * w + 1]), int32"""
    rows = rows.reshape(-1).numpy()
    valid = rows >= 0
    idx = np.full(rows.shape[0], -1, np.int32)
    idx[:int(valid.sum())] = rows[valid]
    return torch.from_numpy(idx), torch.from_numpy(np.concatenate([[0], np.cumsum(valid)]).astype(np.int32))


def _joined_rows(out, name, T, n):
    """the compact CSRs 's<t>_<name>_idx' / '_start' of the T steps joined into one over n slots"""
    valid_rows, starts, off = [], [], 0
    for t in range(T):
        st = out['s%d_%s_start' % (t, name)].numpy()
        valid_rows.append(out['s%d_%s_idx' % (t, name)].numpy()[:int(st[-1])])
        starts.append(st[:-1] + off)
        off += int(st[-1])
    return _pad1np(np.concatenate(valid_rows), n, -1, np.int32), torch.from_numpy(np.concatenate(starts + [[off]]).astype(np.int32))


class EpisodePlanner:
    """TeacherEpisode.plan one step at a time: build_step() makes the host tables of step t from the navigator's current state,
    advance(actions) moves it (the teacher's actions when `imitation`, else the given ones — a sampled rollout decides them from the
    step's logits), finish() adds the joint panorama tables and returns the plan dict.  While a planner is alive it owns te.sim.
    feedback='argmax' (with imitation=False): the validation walk of the reference (M/r2r/agent.py:601-672 under feedback = 'argmax', as
    NavRollout.run does it): action 0 stops, advance() also takes the step's stop scores (and best objects), and a forced end appends the
    backtrack to the node with the best stop score and sets `pred_objid`; self.traj is then the agent's prediction."""

    def __init__(self, te, episodes, imitation=True, feedback=None):
        if feedback not in (None, 'argmax') or (feedback == 'argmax' and imitation):
            raise ValueError('EpisodePlanner: feedback is None or \'argmax\' (the latter with imitation=False), got %r' % (feedback,))
        self.te, self.imitation, self.feedback = te, imitation, feedback
        obs, self.gmaps, self.traj, self.store = start_walk(te.sim, episodes)
        self.B = B = len(obs)
        if feedback == 'argmax':
            self.just_ended = np.zeros(B, bool)
            if te.objects is not None:
                for tr in self.traj:
                    tr['pred_objid'] = None
        lang = language_inputs(obs)
        if lang['txt_ids'].shape[1] > te.L:
            raise ValueError('instruction of %d tokens exceeds the text bucket %d' % (lang['txt_ids'].shape[1], te.L))
        ids = torch.zeros(B, te.L, dtype=torch.int64)
        msk = torch.zeros(B, te.L, dtype=torch.bool)
        ids[:, :lang['txt_ids'].shape[1]], msk[:, :lang['txt_masks'].shape[1]] = lang['txt_ids'], lang['txt_masks']
        self.out = {'txt_ids': ids, 'txt_masks': msk}
        self.obs = obs
        self.ended = np.zeros(B, bool)
        self.n_traj = 0
        self.t = 0
        self._gin = self._target = None

    def build_step(self):
        """-> {key: tensor} of step t (also kept for finish())."""
        from . import graphmap, nav_model       # (lazy: the plan worker imports neither before its first plan)
        te, t, obs, gmaps, ended, store, B = self.te, self.t, self.obs, self.gmaps, self.ended, self.store, self.B
        if t >= te.T:
            raise ValueError('the episode bucket holds %d steps' % te.T)
        afs = te.sim.angle_feat_size
        out = {}
        self.n_traj += int((~ended).sum())
        has_obj = te.objects is not None
        pano = panorama_inputs(obs, afs, te.W, te.O if has_obj else None)
        store.advance(B, te.WT)
        note_step(gmaps, obs, ended, t, store, pano['cand_vpids'])
        G = te.gw(t)
        gin = gmap_inputs(obs, gmaps, G, afs, mem_selectable=has_obj)
        vin = vp_inputs(obs, gmaps, pano['cand_vpids'], pano['view_lens'], pano['nav_types'], te.WT + 2, afs,
                        gmap_pos=(gin['gmap_vpids'], gin['gmap_pos_fts'].numpy()), obj_lens=pano['reverie_obj_lens'] if has_obj else None)
        # (the REVERIE agent has the shortest-path expert only, M/reverie/agent_obj_goat.py:390-417)
        target = teacher_action(obs, gin['gmap_vpids'], ended, gin['gmap_visited_masks'].numpy(), self.imitation and not has_obj, t, te.ignoreid,
                                expert_policy=te.expert_policy, traj=self.traj)
        k = 's%d_' % t
        # feature gather of the panorama tokens: compact CSR (padding slots = empty segments)
        out[k + 'feat_idx'], out[k + 'feat_start'] = _compact_rows(pano['view_rows'])
        for name in ('loc_fts', 'nav_types', 'view_lens'):
            out[k + name] = pano[name]
        for name in ('gmap_step_ids', 'gmap_pos_fts', 'gmap_pair_dists', 'gmap_visited_masks', 'gmap_masks'):
            out[k + name] = gin[name]
        for name in ('vp_pos_fts', 'vp_masks', 'vp_nav_masks'):
            out[k + name] = vin[name]
        if has_obj:
            out[k + 'obj_idx'], out[k + 'obj_start'] = _compact_rows(pano['obj_rows'])
            out[k + 'reverie_obj_lens'], out[k + 'reverie_obj_names'] = pano['reverie_obj_lens'], pano['reverie_obj_names']
            out[k + 'vp_obj_masks'] = vin['vp_obj_masks']
            out[k + 'obj_target'] = torch.from_numpy(teacher_object(obs, ended, pano['view_lens'], te.ignoreid))
            out.update(_obj_concat_tables(pano['view_lens'], pano['reverie_obj_lens'], te.W, te.O, te.WT, k))
        out[k + 'nav_fusion'] = nav_model.nav_fusion_matrix(vin['vp_cand_vpids'], gin['gmap_vpids'], gin['gmap_visited_masks'], G, te.WT + 2)
        # host-side label validation, as train_step.collate_indices does for pre-training (goat_ce_fwd cannot raise; an
        # out-of-range target would only show up as a NaN loss): a teacher action is a map slot of this step or the ignore value
        if ((target >= G) | ((target < 0) & (target != te.ignoreid))).any():
            raise ValueError('teacher action outside the %d map slots of step %d: %s' % (G, t, target.tolist()))
        out[k + 'target'] = torch.from_numpy(target)
        # node embeddings: CSR over the pool of this and all earlier steps (+ the previous [MEM] state behind it)
        n_src = store.rows + (B if t > 0 else 0)
        mem_rows = [store.rows + b for b in range(B)] if t > 0 else None
        idx, start, scale = store.csr(gin['gmap_vpids'], G, mem_rows)
        inv = graphmap.inverse_index(idx, start, scale, n_src)
        n_tok = int(start[-1])
        out[k + 'csr_idx'] = _pad1np(idx[:n_tok] if n_tok else idx[:0], n_src, -1, np.int32)
        out[k + 'csr_start'], out[k + 'csr_scale'] = torch.from_numpy(start), torch.from_numpy(scale)
        out[k + 'inv_idx'] = _pad1np(inv[0].numpy()[:n_tok], n_src, -1, np.int32)
        out[k + 'inv_start'] = inv[1]
        out[k + 'inv_w'] = _pad1np(inv[2].numpy()[:n_tok], n_src, 0.0, np.float32)
        self._gin, self._target = gin, target
        self.out.update(out)
        return out

    def advance(self, actions=None, stop_scores=None, best_obj=None):
        """the move of step t: the teacher's (imitation) or `actions` [B] (indices into the step's map nodes, 0 = [stop]).
        feedback='argmax': stop_scores [B] (the step's softmax[:, 0]) and, with objects, best_obj [B] (index of the best object of the
        current viewpoint) are recorded for the live episodes, as NavRollout.run records them."""
        te, t, obs, gmaps, ended, B = self.te, self.t, self.obs, self.gmaps, self.ended, self.B
        gin, target = self._gin, self._target
        if gin is None:
            raise RuntimeError('advance() before build_step()')
        if not self.imitation and actions is None:
            raise ValueError('a planner of a sampled walk needs the actions of every step')
        argmax = self.feedback == 'argmax'
        if argmax:
            if stop_scores is None or (te.objects is not None and best_obj is None):
                raise ValueError('an argmax walk needs the stop scores (and, with objects, the best objects) of every step')
            for i, g in enumerate(gmaps):
                if not ended[i]:
                    g.node_stop_scores[obs[i]['viewpoint']] = {'stop': float(stop_scores[i])}
                    if te.objects is not None:
                        ids = obs[i]['obj_ids']
                        g.node_stop_scores[obs[i]['viewpoint']]['og'] = ids[int(best_obj[i])] if len(ids) > 0 else None
        moves = []
        for i in range(B):
            stop = (int(actions[i]) == 0) if argmax else (obs[i]['viewpoint'] == obs[i]['gt_path'][-1])
            if stop or ended[i] or gin['no_vp_left'][i] or t == te.T - 1:
                moves.append(None)
                if argmax:
                    self.just_ended[i] = True
                continue
            if self.imitation:
                a = int(target[i])
            else:
                a = int(actions[i])
                if not 0 <= a < len(gin['gmap_vpids'][i]) or (a > 0 and bool(gin['gmap_visited_masks'][i, a])):
                    raise ValueError('step %d, episode %d: recorded action %d is not a navigable node of the map' % (t, i, a))
            nxt = gin['gmap_vpids'][i][a]
            if nxt is None:             # a recorded [stop] (node 0): the episode ends here (M/r2r/agent.py:661)
                moves.append(None)
            else:
                hop = gmaps[i].graph.path(obs[i]['viewpoint'], nxt)
                self.traj[i]['path'].append(hop)
                prev = self.traj[i]['path'][-2][-1] if len(hop) == 1 else hop[-2]
                view = next(c['pointId'] for c in obs[i]['scan_graph'].candidates(prev) if c['viewpointId'] == nxt)
                moves.append((nxt, view))
        if argmax:          # go back to the node with the best stop score (M/r2r/agent.py:665-672; dict order decides ties, as max() there)
            for i in range(B):
                if (not ended[i]) and self.just_ended[i] and gmaps[i].node_stop_scores:
                    stop_node, score = max(gmaps[i].node_stop_scores.items(), key=lambda kv: kv[1]['stop'])
                    if obs[i]['viewpoint'] != stop_node:
                        self.traj[i]['path'].append(gmaps[i].graph.path(obs[i]['viewpoint'], stop_node))
                    if te.objects is not None:
                        self.traj[i]['pred_objid'] = score.get('og')
        self.obs = obs = te.sim.step(moves)
        for i, ob in enumerate(obs):
            if not ended[i]:
                gmaps[i].update_graph(ob)
        self.ended = np.logical_or(ended, np.array([m is None for m in moves]))
        self._gin = self._target = None
        self.t = t + 1

    def finish(self):
        """the plan of the whole episode (every step built and advanced)."""
        te, out, B = self.te, self.out, self.B
        if self.t != te.T:
            raise RuntimeError('finish() after %d of %d steps' % (self.t, te.T))
        # the panoramas of all steps as ONE batch [T * B] (body(hoist_pano=True)): the compact feature-gather CSR of the steps joined
        out['all_feat_idx'], out['all_feat_start'] = _joined_rows(out, 'feat', te.T, te.T * B * te.W)
        for name in ('loc_fts', 'nav_types', 'view_lens'):
            out['all_' + name] = torch.cat([out['s%d_%s' % (t, name)] for t in range(te.T)], 0)
        if te.objects is not None:
            out['all_obj_idx'], out['all_obj_start'] = _joined_rows(out, 'obj', te.T, te.T * B * te.O)
            for name in ('reverie_obj_lens', 'reverie_obj_names'):
                out['all_' + name] = torch.cat([out['s%d_%s' % (t, name)] for t in range(te.T)], 0)
            out.update(_obj_concat_tables(out['all_view_lens'], out['all_reverie_obj_lens'], te.W, te.O, te.WT, 'all_'))
        out['_traj'], out['_n_traj'] = self.traj, self.n_traj
        return out


class _RowIndex:
    """key -> row lookup of a feature store without its table (what GraphSim needs of it on the host)."""

    def __init__(self, keys):
        self.index = {k: i for i, k in enumerate(keys)}

    def row(self, scan, vp):
        return self.index['%s_%s' % (scan, vp)]


def _plan_worker_main(conn, spec):
    os.environ.setdefault('HIP_VISIBLE_DEVICES', '-1')        # host work only: the worker never touches the GPU
    torch.set_num_threads(1)          # small host tensors only: the default intra-op pool (one thread per core: 128-256 on the GPU boxes) costs
                                      # tens of ms in wake-ups per plan (measured: 60 ms per plan with the pool, 13 ms without)
    scans = spec['scans']
    te = TeacherEpisode(GraphSim(_RowIndex(spec['keys']), spec['angle_feat_size'], objects=spec.get('objects')), None, spec['n_steps'],
                        spec['text_len'], pano_width=spec['pano_width'], gmap_width=lambda t, w=spec['gmap_widths']: w[min(t, len(w) - 1)],
                        fusion=spec['fusion'], ignoreid=spec['ignoreid'], obj_width=spec.get('obj_width', 20),
                        expert_policy=spec.get('expert_policy', 'spl'))
    while True:
        try:
            episodes = conn.recv()
        except EOFError:
            break
        if episodes is None:
            break
        try:
            t0 = time.perf_counter()
            plan = te.plan([dict(e, scan=scans[e['scan']]) for e in episodes])
            plan['_plan_s'] = time.perf_counter() - t0
            plan.pop('_traj', None)
            # numpy through the pipe: torch tensors would travel as one shared-memory segment + file descriptor EACH (~150 per plan: 10 ms)
            conn.send({k: (('__t', v.numpy()) if torch.is_tensor(v) else v) for k, v in plan.items()})
        except Exception as e:      # noqa: BLE001  (reported to the caller, the worker stays alive)
            conn.send(e)


class PlanWorker:
    """TeacherEpisode.plan in a worker PROCESS.  The plan of a batch of episodes is 10-15 ms of pure-Python table building; next to it the
    training process copies the previous plan into the pinned buffer and launches a ~3 000-node episode graph (several ms of host time in
    hipGraphLaunch).  A thread does not help (the builders hold the GIL: 21-24 ms per episode against 19 ms of GPU work); a process does.
    submit(episodes) returns at once (the episodes travel with their scan NAMES; the worker holds the ScanGraphs, its own GraphSim over the
    store's key -> row map, and never initialises the GPU — spawn context, safe beside an initialised HIP runtime); a reader thread of this
    process drains the worker's pipe (plans are ~3 MB: a worker blocked in send while this process blocks in submit would deadlock);
    result() hands back the next plan dict (CPU tensors) in submission order.

        pw = PlanWorker(te, store.keys, scans);  pw.submit(eps_0); pw.submit(eps_1)          # two in flight
        for k in ...:  plan = pw.result(); pw.submit(eps_k2); bufs.load(plan); graph.replay()"""

    def __init__(self, te, keys, scans):
        ctx = mp.get_context('spawn')
        self.conn, child = ctx.Pipe()
        scans = {sc.name: sc for sc in (scans.values() if isinstance(scans, dict) else scans)}
        spec = {'keys': list(keys), 'scans': scans, 'angle_feat_size': te.sim.angle_feat_size, 'n_steps': te.T, 'text_len': te.L,
                'pano_width': te.W, 'gmap_widths': [int(te.gw(t)) for t in range(max(te.T, 1))], 'fusion': te.fusion, 'ignoreid': te.ignoreid,
                'objects': te.objects.meta() if te.objects is not None else None, 'obj_width': te.O, 'expert_policy': te.expert_policy}      # (REVERIE: object metadata, no features)
        self.proc = ctx.Process(target=_plan_worker_main, args=(child, spec), daemon=True)
        self.proc.start()
        child.close()
        self.pending = 0
        self._q = queue.Queue()

        def drain():
            while True:
                try:
                    self._q.put(self.conn.recv())
                except (EOFError, OSError):
                    self._q.put(EOFError('plan worker exited'))
                    return
        self._reader = threading.Thread(target=drain, daemon=True)
        self._reader.start()

    def submit(self, episodes):
        self.conn.send([dict(e, scan=e['scan'].name if not isinstance(e['scan'], str) else e['scan']) for e in episodes])
        self.pending += 1

    def result(self, timeout=120.0):
        if self.pending <= 0:
            raise RuntimeError('PlanWorker.result() without a submitted batch of episodes')
        try:
            plan = self._q.get(timeout=timeout)
        except queue.Empty:
            raise TimeoutError('plan worker (pid %s, %s) returned no plan within %.0f s'
                               % (self.proc.pid, 'alive' if self.proc.is_alive() else 'exited', timeout)) from None
        self.pending -= 1
        if isinstance(plan, Exception):
            raise plan
        return {k: (torch.from_numpy(v[1]) if (isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str) and v[0] == '__t') else v)
                for k, v in plan.items()}

    def close(self):
        """stop the worker (idempotent); plans not yet fetched are dropped."""
        if self.proc is None:
            return
        try:
            self.conn.send(None)
        except (OSError, BrokenPipeError):
            pass
        self.proc.join(5)
        if self.proc.is_alive():
            self.proc.terminate()
            self.proc.join(5)
        self.conn.close()
        self.proc = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _pad1np(a, n, fill, dtype):
    out = np.full(n, fill, dtype)
    out[:len(a)] = a
    return torch.from_numpy(out)


class EpisodeBuffers:
    """the tensors of a TeacherEpisode.plan at FIXED device addresses (one flat buffer; one pinned H2D copy per new plan)."""
    ALIGN = 256

    def __init__(self, plan, device='cuda'):
        self.device = torch.device(device)
        self.layout, off = [], 0
        for k in sorted(plan):
            v = plan[k]
            if torch.is_tensor(v):
                self.layout.append((k, off, tuple(v.shape), v.dtype))
                off += (v.numel() * v.element_size() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self._where = {k: (off, shape, dtype) for k, off, shape, dtype in self.layout}
        self.nbytes = max(off, self.ALIGN)
        self.flat = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)
        self.host = torch.zeros(self.nbytes, dtype=torch.uint8)
        if self.device.type == 'cuda':
            self.host = self.host.pin_memory()
        self.t = {}
        for k, off, shape, dtype in self.layout:
            n = 1
            for s in shape:
                n *= s
            self.t[k] = self.flat[off:off + n * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(shape)
        self._copied = None
        self.load(plan)

    def load_part(self, part):
        """the tensors of `part` only (e.g. EpisodePlanner.build_step(): the tables of one step): packed into the pinned buffer, ONE H2D of
        the byte range that covers them (the bytes between them are what the device already holds), their memoised masks refreshed."""
        if self._copied is not None:
            self._copied.synchronize()
        where = self._where
        dst = self.host.numpy()
        lo, hi = self.nbytes, 0
        for k, v in part.items():
            if not torch.is_tensor(v):
                continue
            off, shape, dtype = where[k]
            if tuple(v.shape) != shape or v.dtype != dtype:
                raise ValueError('EpisodeBuffers: %s is %s %s, the captured layout has %s %s' % (k, tuple(v.shape), v.dtype, shape, dtype))
            n = v.numel() * v.element_size()
            if n:
                dst[off:off + n] = v.contiguous().view(-1).view(torch.uint8).numpy()
                lo, hi = min(lo, off), max(hi, off + n)
        if hi > lo:
            self.flat[lo:hi].copy_(self.host[lo:hi], non_blocking=True)
            if self.device.type == 'cuda':
                self._copied = torch.cuda.Event()
                self._copied.record()
        layers.refresh_masks(only=[self.t[k] for k in part if k in self.t])

    def load(self, plan, stream=None):
        """pack `plan` into the pinned buffer and copy it to the device (asynchronously on `stream` / the current stream)."""
        if self._copied is not None:
            self._copied.synchronize()              # the previous H2D has read the pinned buffer
        dst = self.host.numpy()
        for k, off, shape, dtype in self.layout:
            v = plan.get(k)
            if v is None or tuple(v.shape) != shape or v.dtype != dtype:
                raise ValueError('EpisodeBuffers: %s is %s %s, the captured layout has %s %s'
                                 % (k, None if v is None else tuple(v.shape), None if v is None else v.dtype, shape, dtype))
            n = v.numel() * v.element_size()
            if n:
                dst[off:off + n] = v.contiguous().view(-1).view(torch.uint8).numpy()
        if stream is not None:
            with torch.cuda.stream(stream):
                self.flat.copy_(self.host, non_blocking=True)
        else:
            self.flat.copy_(self.host, non_blocking=True)
        if self.device.type == 'cuda':
            self._copied = torch.cuda.Event()
            self._copied.record(stream)
        layers.refresh_masks()
