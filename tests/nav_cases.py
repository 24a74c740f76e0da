"""The bench every device-navigator test stands on (the CPU tests of the kernels' text and the GPU tests of navdev.DeviceNavigator): the
episode bucket over synthetic scans, ONE host walk of EpisodePlanner that records the tables, actions and counts the tests'
preconditions ask for, the random policy, the table comparison and the driver of a DeviceNavigator under the host's actions.  The
cases, policies and preconditions of the nDTW expert and of the object walks are in ndtw_cases.py and object_nav_cases.py.  Nothing
here needs a GPU."""
from types import SimpleNamespace

import numpy as np
import torch

A = 4
TABLES = ('feat_idx', 'feat_start', 'loc_fts', 'nav_types', 'view_lens', 'gmap_step_ids', 'gmap_pos_fts', 'gmap_pair_dists', 'gmap_visited_masks',
          'gmap_masks', 'vp_pos_fts', 'vp_masks', 'vp_nav_masks', 'nav_fusion', 'target', 'csr_idx', 'csr_start', 'csr_scale', 'inv_idx', 'inv_start',
          'inv_w')
OBJECT_TABLES = ('obj_idx', 'obj_start', 'reverie_obj_lens', 'reverie_obj_names', 'vp_obj_masks', 'obj_target', 'ocat_idx', 'ocat_start',
                 'ocat_inv_idx', 'ocat_inv_start')
# columns that go through sin / cos / asin (and the line distance): 1e-6; every other column exact.  The angle columns of loc_fts include
# those of the object rows.
LOOSE = {'loc_fts': list(range(A)), 'gmap_pos_fts': list(range(A + 1)), 'vp_pos_fts': list(range(A + 1)) + [A + 3 + c for c in range(A + 1)]}
EP_ARGS = dict(num_l_layers=2, num_x_layers=2, num_pano_layers=2, dropout=0.5, feat_dropout=0.4, do_back_img=True, do_back_txt=True,
               do_front_img=True, do_front_his=True, do_front_txt=True, vocab_size=1200, mode='train', do_back_txt_type='type_2',
               do_back_img_type='type_1', do_add_method='door')


def bench(scans, T, gmap_width=None, objects=None, obj_fallback=False, W=40, **te_kw):
    """sim over a key -> row index of `scans` (objects: the metadata of an ObjectStore) and the episode bucket; te_kw: expert_policy,
    obj_width"""
    from vln_goat_amd import rollout
    keys = ['%s_%s' % (sc.name, vp) for sc in scans for vp in sc.vpids]
    sim = rollout.GraphSim(rollout._RowIndex(keys)) if objects is None else rollout.GraphSim(rollout._RowIndex(keys), objects=objects, obj_fallback=obj_fallback)
    if gmap_width is not None:
        te_kw['gmap_width'] = gmap_width
    return sim, rollout.TeacherEpisode(sim, None, n_steps=T, text_len=32, pano_width=W, **te_kw)


def random_policy(seed, p_stop, scores=True):
    """a random selectable node, or with p_stop [stop] -> (actions, stop scores drawn from the same stream | None)"""
    rs = np.random.RandomState(seed)

    def policy(t, p, part):
        sel = (part['s%d_gmap_masks' % t] & ~part['s%d_gmap_visited_masks' % t]).numpy()
        a = np.zeros(p.B, np.int64)
        for b in range(p.B):
            stop = rs.uniform() < p_stop
            slots = np.nonzero(sel[b, 2:])[0] + 2
            pick = int(slots[rs.randint(len(slots))]) if len(slots) else 0
            a[b] = 0 if (stop or p.ended[b]) else pick
        return a, (rs.uniform(0.05, 0.95, p.B).astype(np.float32) if scores else None)
    return policy


def host_walk(te, eps, policy, feedback=None, observe=None):
    """The host planner driven by policy(t, planner, part) -> actions [B] | (actions, stop scores [B] | None[, best objects [B]]).
    observe(t, planner, part, stats): what a case counts on the state of step t before the move.  -> parts (the tables of every step),
    acts, scores, bests, ended (the flags after every move), p (the planner) and stats: moves, multi-hop moves, live states with no node
    left, averaged node embeddings, map rows with several fusion entries, and what `observe` added."""
    from vln_goat_amd import rollout
    p = rollout.EpisodePlanner(te, eps, imitation=False, feedback=feedback)
    w = SimpleNamespace(parts=[], acts=[], scores=[], bests=[], ended=[], p=p, stats={'multi': 0, 'moves': 0, 'noleft': 0, 'avg': 0, 'fusion_rows': 0})
    for t in range(te.T):
        part = {k: v.clone() for k, v in p.build_step().items()}
        if observe is not None:
            observe(t, p, part, w.stats)
        out = policy(t, p, part)
        a, s, o = (tuple(out) + (None, None))[:3] if isinstance(out, tuple) else (out, None, None)
        w.stats['noleft'] += int(sum(bool(x) and l for x, l in zip(p._gin['no_vp_left'], ~p.ended)))
        w.stats['avg'] += int((part['s%d_csr_scale' % t] < 1).sum())
        w.stats['fusion_rows'] += int(((part['s%d_nav_fusion' % t] > 0).sum(2) > 1).sum())
        before = [len(tr['path']) for tr in p.traj]
        if feedback == 'argmax':
            p.advance(a, s, o)
        else:
            p.advance(a)
        for tr, n in zip(p.traj, before):
            for hop in tr['path'][n:n + 1]:
                w.stats['moves'] += 1
                w.stats['multi'] += len(hop) > 1
        w.parts.append(part)
        w.acts.append(np.asarray(a, np.int64))
        w.scores.append(None if s is None else np.asarray(s, np.float32))
        w.bests.append(None if o is None else np.asarray(o, np.float32))
        w.ended.append(p.ended.copy())
    return w


def compare(t, got, want, tables=TABLES):
    """every table of step t, padding included (got: {key: tensor} on any device)"""
    for name in tables:
        k = 's%d_%s' % (t, name)
        g, w = got[k].cpu(), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if name in LOOSE:
            loose = torch.zeros(g.shape[-1], dtype=torch.bool)
            loose[LOOSE[name]] = True
            assert torch.equal(g[..., ~loose], w[..., ~loose]), k
            err = float((g[..., loose] - w[..., loose]).abs().max())
            assert err <= 1e-6, (k, err)
        else:
            assert torch.equal(g, w), (k, g.reshape(-1)[:48], w.reshape(-1)[:48])


def back_rows(w, t):
    """the [3, B] float32 tensor an argmax step graph leaves for the move of step t: actions, stop scores, best objects (zeros without)"""
    best = w.bests[t] if w.bests[t] is not None else np.zeros(len(w.acts[t]), np.float32)
    return np.stack([w.acts[t].astype(np.float32), w.scores[t], best])


def device_walk(nav, eps, bufs, w, mode='forced', tables=TABLES):
    """the navigator over `bufs` under the actions (argmax: and stop scores / best objects) of the host walk `w`; every step's tables
    against the host's -> nav.finish(): (traj, actions, n_traj, ended)"""
    back = torch.zeros(3, len(eps), dtype=torch.float32, device=bufs.device)
    nav.begin(eps, actions=w.acts if mode == 'forced' else None)
    for t in range(nav.T + 1):
        if t > 0 and mode == 'argmax':
            back.copy_(torch.from_numpy(back_rows(w, t - 1)))
        nav.step(t, back if mode == 'argmax' else None)
        if t < nav.T:
            if bufs.device.type == 'cuda':
                torch.cuda.synchronize()
            compare(t, bufs.t, w.parts[t], tables)
    return nav.finish()


def same_walk(got, p):
    """trajectories, instruction ids, n_traj and the ended flags of nav.finish() against the planner's"""
    traj, actions, n_traj, ended = got
    assert [tr['path'] for tr in traj] == [tr['path'] for tr in p.traj]
    assert [tr['instr_id'] for tr in traj] == [tr['instr_id'] for tr in p.traj]
    assert n_traj == p.n_traj and np.array_equal(ended, p.ended)


class FixedRng:
    def __init__(self, u):
        self.u = u

    def random_sample(self, n):
        return self.u


def check_sampling(probs, u, actions, alive):
    """the recorded action of every live episode equals SampledEpisode.sample on the host from the same probs and uniform -> how many"""
    from vln_goat_amd import rollout
    n = 0
    for t in range(len(probs)):
        want = rollout.SampledEpisode.sample(probs[t], FixedRng(u[t]))
        for b in range(probs[t].shape[0]):
            if alive[t, b]:
                assert actions[t][b] == want[b], (t, b, actions[t][b], want[b])
                n += 1
    return n


def masks_match():
    """every memoised mask equals its recomputation from the table it was derived from -> how many"""
    from vln_goat_amd import layers
    n = 0
    for ent in layers._MASK_MEMO.values():
        src = ent[0]()
        if src is not None:
            assert torch.equal(ent[2], ent[3](src)), ent[2].shape
            n += 1
    return n
