"""The host input builders of the fine-tuning rollout (overview: rollout.py) and the few steps every walk shares.  Built on
navsim.py; used by rollout.py, episodes.py and sampled.py, never the other way round.

  * `panorama_inputs`, `gmap_inputs`, `vp_inputs`, `teacher_action`   the builders of M/r2r/agent.py:82-148,151-237,271-304,306-347,
                                  producing the `panorama` / `navigation` input dicts of VLNBert.forward — small integer / float32
                                  tables built by numpy on the host; the 36 x 768 view features are never touched on the host: the
                                  builders emit ROW INDICES into a device-resident feature table (features.FeatureStore) and one
                                  gather kernel assembles the batch in HBM.
  * `start_walk`, `note_step`, `nodefault`, `fused_or_mean`, `pick_logits`   what NavRollout and the planned episodes share."""
from collections import defaultdict

import numpy as np
import torch

from .navsim import GraphMap, NodeEmbedStore


# ------------------------------------------------------------------------------------------------ input builders (agent.py)
def language_inputs(obs, pad_id=0):
    """_language_variable (M/r2r/agent.py:38-65) without the dictionaries (the caller adds the BACL / FACL tensors)."""
    lens = [len(ob['instr_encoding']) for ob in obs]
    ids = np.full((len(obs), max(lens)), pad_id, np.int64)
    mask = np.zeros((len(obs), max(lens)), bool)
    for i, ob in enumerate(obs):
        ids[i, :lens[i]] = ob['instr_encoding']
        mask[i, :lens[i]] = True
    return {'txt_ids': torch.from_numpy(ids), 'txt_masks': torch.from_numpy(mask)}


def panorama_inputs(obs, angle_feat_size=4, width=None, obj_width=None):
    """_panorama_feature_variable_do (M/r2r/agent.py:82-148): candidate views first (nav type 1), then the views no candidate
    used (nav type 0), padded to the longest panorama of the batch (or `width`).  The 768-wide image features are NOT assembled
    here: `view_rows[b, j]` = feature_row * 36 + view index of token j (-1: padding) for a device gather."""
    B = len(obs)
    rows, locs, types, cand_vpids, lens = [], [], [], [], []
    for ob in obs:
        used, r, ang, ty, cv = set(), [], [], [], []
        for cc in ob['candidate']:
            r.append(ob['feature_row'] * 36 + cc['pointId'])
            ang.append(cc['angle_feat'])
            ty.append(1)
            cv.append(cc['viewpointId'])
            used.add(cc['pointId'])
        rest = [k for k in range(36) if k not in used]
        base = ob['feature_row'] * 36
        r.extend(base + k for k in rest)
        ty.extend([0] * len(rest))
        loc = np.ones((len(r), angle_feat_size + 3), np.float32)
        if ang:
            loc[:len(ang), :angle_feat_size] = np.stack(ang, 0)
        loc[len(ang):, :angle_feat_size] = np.asarray(ob['view_angle_fts'])[rest]
        locs.append(loc)
        rows.append(r)
        types.append(ty)
        cand_vpids.append(cv)
        lens.append(len(r))
    W = max(lens) if width is None else width
    if W < max(lens):
        raise ValueError('panorama_inputs: a panorama has %d tokens, the bucket holds %d' % (max(lens), W))
    view_rows = np.full((B, W), -1, np.int64)
    loc_fts = np.zeros((B, W, angle_feat_size + 3), np.float32)
    nav_types = np.zeros((B, W), np.int64)
    for b in range(B):
        view_rows[b, :lens[b]] = rows[b]
        loc_fts[b, :lens[b]] = locs[b]
        nav_types[b, :lens[b]] = types[b]
    out = {'view_rows': torch.from_numpy(view_rows), 'loc_fts': torch.from_numpy(loc_fts), 'nav_types': torch.from_numpy(nav_types),
           'view_lens': torch.tensor(lens, dtype=torch.int64), 'cand_vpids': cand_vpids}
    if 'obj_ids' in obs[0]:
        out.update(panorama_object_inputs(obs, out, angle_feat_size, obj_width))
    return out


def panorama_object_inputs(obs, pano, angle_feat_size=4, obj_width=None):
    """The object half of `_panorama_feature_variable_do` of the REVERIE agent (M/reverie/agent_obj_goat.py:180-271): object tokens follow
    the views of their panorama (nav type 2), `loc_fts` / `nav_types` cover views + objects (padded to the longest row of the batch),
    `reverie_obj_*` are the per-object tensors the image embedding consumes.  obj_rows[b, j] = row of ObjectStore.table (-1: padding)."""
    B = len(obs)
    A = angle_feat_size + 3
    olens = [len(ob['obj_ids']) for ob in obs]
    vlens = [int(x) for x in pano['view_lens']]
    O = max(olens) if obj_width is None else obj_width
    if O < max(olens):
        raise ValueError('panorama_object_inputs: a viewpoint has %d objects, the bucket holds %d' % (max(olens), O))
    Wv = pano['view_rows'].shape[1]
    W = max(v + o for v, o in zip(vlens, olens)) if obj_width is None else Wv + O
    obj_rows = np.full((B, O), -1, np.int64)
    obj_locs = np.zeros((B, O, A), np.float32)
    obj_names = np.zeros((B, O), np.int64)
    loc_fts = np.zeros((B, W, A), np.float32)
    nav_types = np.zeros((B, W), np.int64)
    rnav = np.zeros((B, 36 + O), np.int64)
    vloc, vty = pano['loc_fts'].numpy(), pano['nav_types'].numpy()
    for b, ob in enumerate(obs):
        v, o = vlens[b], olens[b]
        loc_fts[b, :v], nav_types[b, :v] = vloc[b, :v], vty[b, :v]
        if o:
            ol = np.concatenate([ob['obj_ang_fts'], ob['obj_box_fts']], 1)
            obj_rows[b, :o], obj_locs[b, :o], obj_names[b, :o] = ob['obj_rows'], ol, np.asarray(ob['obj_name'], np.int64)
            loc_fts[b, v:v + o], nav_types[b, v:v + o] = ol, 2
            rnav[b, 36:36 + o] = 2
    return {'loc_fts': torch.from_numpy(loc_fts), 'nav_types': torch.from_numpy(nav_types), 'obj_rows': torch.from_numpy(obj_rows),
            'reverie_obj_lens': torch.tensor(olens, dtype=torch.int64), 'reverie_obj_locs': torch.from_numpy(obj_locs),
            'reverie_obj_names': torch.from_numpy(obj_names), 'reverie_obj_nav_types': torch.from_numpy(rnav),
            'obj_ids': [list(ob['obj_ids']) for ob in obs]}


def gmap_order(gmap):
    """[stop], [MEM], visited nodes, unvisited nodes in the insertion order of node_positions (M/r2r/agent.py:159-176,
    enc_full_graph)."""
    visited = [k for k in gmap.node_positions if gmap.graph.visited(k)]
    unvisited = [k for k in gmap.node_positions if not gmap.graph.visited(k)]
    return [None, None] + visited + unvisited, [0, 1] + [1] * len(visited) + [0] * len(unvisited), len(unvisited) == 0


def gmap_inputs(obs, gmaps, width=None, angle_feat_size=4, mem_selectable=False):
    """_nav_gmap_variable (M/r2r/agent.py:151-237) without the embeddings (NodeEmbedStore.gather)."""
    B = len(obs)
    vpids, vis, no_left = zip(*[gmap_order(g) for g in gmaps])
    lens = [len(v) for v in vpids]
    G = max(lens) if width is None else width
    if G < max(lens):
        raise ValueError('gmap_inputs: a map has %d nodes, the bucket holds %d' % (max(lens), G))
    step_ids = np.zeros((B, G), np.int64)
    pos = np.zeros((B, G, angle_feat_size + 3), np.float32)
    pair = np.zeros((B, G, G), np.float32)
    vmask = np.zeros((B, G), bool)
    gmask = np.zeros((B, G), bool)
    for b, (ob, g) in enumerate(zip(obs, gmaps)):
        n = lens[b]
        step_ids[b, :n] = [g.node_step_ids.get(vp, 0) for vp in vpids[b]]
        pos[b, :n] = g.get_pos_fts(ob['viewpoint'], vpids[b], ob['heading'], ob['elevation'], angle_feat_size)
        pair[b, :n, :n] = g.pair_dists(vpids[b])
        vmask[b, :n] = np.asarray(vis[b], bool)
        gmask[b, :n] = True
    if not mem_selectable:              # the [MEM] token cannot be chosen (M/r2r/agent.py:209).  The REVERIE agent's copy of this builder lacks
        gmask[:, 1] = False             # that line (M/reverie/agent_obj_goat.py:273-343): there the slot stays selectable (its viewpoint id is
                                        # None: choosing it ends the episode like [stop]) — mem_selectable=True reproduces it
    return {'gmap_vpids': [list(v) for v in vpids], 'gmap_step_ids': torch.from_numpy(step_ids), 'gmap_pos_fts': torch.from_numpy(pos),
            'gmap_visited_masks': torch.from_numpy(vmask), 'gmap_pair_dists': torch.from_numpy(pair), 'gmap_masks': torch.from_numpy(gmask),
            'gmap_lens': lens, 'no_vp_left': list(no_left)}


def vp_inputs(obs, gmaps, cand_vpids, view_lens, nav_types, width, angle_feat_size=4, gmap_pos=None, obj_lens=None):
    """_nav_vp_variable_mem (M/r2r/agent.py:271-304) without the embeddings: [stop], [MEM], then the panorama tokens.
    width = panorama width + 2.  gmap_pos = (gmap_vpids, gmap_pos_fts [B, G, angle_feat_size + 3]) of gmap_inputs on the SAME
    observations: the candidates and the start node are nodes of the map and their features are seen from the same viewpoint under
    the same heading — the rows are taken from there instead of being computed a second and third time."""
    B = len(obs)
    A = angle_feat_size + 3
    pos = np.zeros((B, width, 2 * A), np.float32)
    for b, (ob, g) in enumerate(zip(obs, gmaps)):
        if gmap_pos is not None:
            where = {vp: j for j, vp in enumerate(gmap_pos[0][b]) if vp is not None}
            rows = gmap_pos[1][b]
            cand = rows[[where[vp] for vp in cand_vpids[b]]] if cand_vpids[b] else np.zeros((0, A), np.float32)
            start = rows[where[g.start_vp]]
        else:
            cand = g.get_pos_fts(ob['viewpoint'], cand_vpids[b], ob['heading'], ob['elevation'], angle_feat_size) if cand_vpids[b] else \
                np.zeros((0, A), np.float32)
            start = g.get_pos_fts(ob['viewpoint'], [g.start_vp], ob['heading'], ob['elevation'], angle_feat_size)
        pos[b, :, :A] = start
        pos[b, 2:len(cand) + 2, A:] = cand
    nav_types = torch.as_tensor(nav_types)
    view_lens = torch.as_tensor(view_lens)
    head = [torch.ones(B, 1, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)]
    out = {'vp_pos_fts': torch.from_numpy(pos), 'vp_masks': torch.arange(width)[None, :] < (view_lens + 2)[:, None],
           'vp_nav_masks': torch.cat(head + [nav_types == 1], 1), 'vp_cand_vpids': [[None, None] + list(x) for x in cand_vpids]}
    if obj_lens is not None:        # REVERIE (_nav_vp_variable_do, M/reverie/agent_obj_goat.py:345-388): object tokens behind the views
        out['vp_masks'] = torch.arange(width)[None, :] < (view_lens + torch.as_tensor(obj_lens) + 2)[:, None]
        out['vp_obj_masks'] = torch.cat(head + [nav_types == 2], 1)
    return out


def teacher_object(obs, ended, view_lens, ignoreid=-100):
    """_teacher_object (M/reverie/agent_obj_goat.py:419-436): at a goal viewpoint the index of the target object among the local tokens
    ([stop], [MEM], views, objects); everywhere else — and when the target is not among the detected objects — the ignore value."""
    t = np.full(len(obs), ignoreid, np.int64)
    for i, ob in enumerate(obs):
        if ended[i] or ob['viewpoint'] not in ob['gt_end_vps']:
            continue
        for j, oid in enumerate(ob['obj_ids']):
            if str(oid) == str(ob['gt_obj_id']):
                t[i] = j + int(view_lens[i]) + 2
                break
    return t


EXPERT_POLICIES = ('spl', 'ndtw')


def cal_dtw(dist, prediction, reference, threshold=3.0):
    """cal_dtw (M/r2r/eval_utils.py:6-26) over a dense distance matrix: prediction / reference are rows / columns of `dist` (indices of
    `ScanGraph.vpids`).  The loops, their order and the float64 operations are the reference's; -> {'DTW', 'nDTW'}."""
    dtw_matrix = np.inf * np.ones((len(prediction) + 1, len(reference) + 1))
    dtw_matrix[0][0] = 0
    for i in range(1, len(prediction) + 1):
        for j in range(1, len(reference) + 1):
            best_previous_cost = min(dtw_matrix[i - 1][j], dtw_matrix[i][j - 1], dtw_matrix[i - 1][j - 1])
            cost = dist[prediction[i - 1]][reference[j - 1]]
            dtw_matrix[i][j] = cost + best_previous_cost
    dtw = dtw_matrix[len(prediction)][len(reference)]
    return {'DTW': dtw, 'nDTW': np.exp(-dtw / (threshold * len(reference)))}


def teacher_action(obs, vpids, ended, visited_masks=None, imitation_learning=False, t=None, ignoreid=-100, expert_policy='spl', traj=None):
    """_teacher_action (M/r2r/agent.py:306-347).  expert_policy (imitation_learning=False): 'spl', the unvisited node with the shortest
    way to the goal through it, or 'ndtw' (:330-346, the RxR scripts), the unvisited node whose shortest path from the current
    viewpoint, appended to the walked path `traj[i]['path']`, keeps the highest nDTW to the ground-truth path.  Shortest paths are
    `ScanGraph.shortest_path` (the reference takes networkx's)."""
    if expert_policy not in EXPERT_POLICIES:
        raise ValueError('teacher_action: expert_policy is one of %s, got %r' % (EXPERT_POLICIES, expert_policy))
    if expert_policy == 'ndtw' and not imitation_learning and traj is None:
        raise ValueError('teacher_action: the ndtw expert scores the walked path: pass traj')
    a = np.zeros(len(obs), dtype=np.int64)
    for i, ob in enumerate(obs):
        if ended[i]:
            a[i] = ignoreid
        elif imitation_learning:
            assert ob['viewpoint'] == ob['gt_path'][t]
            if t == len(ob['gt_path']) - 1:
                a[i] = 0
            else:
                goal = ob['gt_path'][t + 1]
                for j, vpid in enumerate(vpids[i]):
                    if goal == vpid:
                        a[i] = j
                        break
        elif ob['viewpoint'] == ob['gt_path'][-1]:
            a[i] = 0
        else:
            scan = ob['scan_graph']
            dist, _ = scan.shortest()
            cur, goal = scan.index[ob['viewpoint']], scan.index[ob['gt_path'][-1]]
            best, best_d = ignoreid, float('inf')
            if expert_policy == 'ndtw':
                walked = [scan.index[vp] for vp in sum(traj[i]['path'], [])]
                gt = [scan.index[vp] for vp in ob['gt_path']]
            for j, vpid in enumerate(vpids[i]):
                if j > 1 and ((visited_masks is None) or (not visited_masks[i][j])):
                    k = scan.index[vpid]
                    if expert_policy == 'ndtw':
                        there = [scan.index[vp] for vp in scan.shortest_path(ob['viewpoint'], vpid)[1:]]
                        d = -cal_dtw(dist, walked + there, gt, threshold=3.0)['nDTW']
                    else:
                        d = dist[k, goal] + dist[cur, k]
                    if d < best_d:
                        best_d, best = d, j
            a[i] = best
    return a


# ------------------------------------------------------------------------------------------------ shared by every walk
def start_walk(sim, episodes):
    """reset the navigator and open one map per episode (M/r2r/agent.py:448-470) -> (obs, gmaps, traj, NodeEmbedStore)"""
    obs = sim.reset(episodes)
    gmaps = [GraphMap(ob['viewpoint']) for ob in obs]
    for g, ob in zip(gmaps, obs):
        g.update_graph(ob)
    traj = [{'instr_id': ob['instr_id'], 'path': [[ob['viewpoint']]]} for ob in obs]
    return obs, gmaps, traj, NodeEmbedStore(len(obs))


def note_step(gmaps, obs, ended, t, store, cand_vpids):
    """map bookkeeping of step t for the episodes still walking (M/r2r/agent.py:557-573), after the store has registered the step's
    panorama rows: the step id of the current node, its embedding rewritten by this visit, the unvisited candidates accumulated."""
    for i, g in enumerate(gmaps):
        if not ended[i]:
            vp = obs[i]['viewpoint']
            g.node_step_ids[vp] = t + 1
            store.rewrite(i, vp)
            for j, cvp in enumerate(cand_vpids[i]):
                if not g.graph.visited(cvp):
                    store.accumulate(i, cvp, j)


def nodefault(d):
    """the input dict of a model call: a key the caller did not set reads as None"""
    return defaultdict(lambda: None, d)


def fused_or_mean(pano, pmask, fused):
    """the panorama vector [B, H]: the model's fused one, or without adaptive_pano_fusion the masked mean (M/r2r/agent.py:545-547)"""
    if fused is None:
        fused = torch.sum(pano * pmask.unsqueeze(2), 1) / torch.sum(pmask, 1, keepdim=True)
    return fused


def pick_logits(out, fusion):
    """the logits of the configured fusion ('local' / 'global' / anything else: the fused ones) of a navigation output"""
    return {'local': out['local_logits'], 'global': out['global_logits']}.get(fusion, out['fused_logits'])
