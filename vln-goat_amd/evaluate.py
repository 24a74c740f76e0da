"""Validation on the device: the reference's `eval_metrics` (M/r2r/env.py:452-520, M/reverie/env.py:530-581) without MatterSim.

The reference scores every predicted trajectory in Python loops over dict-of-dict distance tables: DTW and CLS are O(P R) lookups
per item (M/r2r/eval_utils.py).  Here the distance tables of all scans live in ONE float64 device buffer, the predictions of a whole
split are flattened to node indices on the host, and `goat_nav_metrics` (csrc/navmetrics.hip) scores all of them in one launch.

  * `ScanDistances`     the `ScanGraph.shortest()[0]` tables of a list of scans packed into one device buffer.
  * `NavEvaluator`      `eval_metrics(preds)` of both agents (R2R: SR / SPL / oracle SR / nDTW / SDTW / CLS; REVERIE with `obj2vps`:
                        the goal-viewpoint success rule plus RGS / RGSPL): one upload, one launch, one read-back.
  * `validate`          the argmax walk (`rollout.ArgmaxEpisode`) over batches of episodes, then `eval_metrics` once."""
import numpy as np
import torch

from ._plumbing import launch

COLS = ('nav_error', 'oracle_error', 'trajectory_steps', 'trajectory_lengths', 'gt_lengths', 'success', 'oracle_success', 'spl', 'DTW',
        'nDTW', 'SDTW', 'CLS')
MAX_REF = 2047          # goat_nav_metrics keeps three DTW diagonals of the reference path in LDS


class ScanDistances:
    """The all-pairs shortest distances of `scans` (ScanGraph objects) as one packed float64 device buffer: scan k owns the row-major
    [n_k, n_k] block at `off[k]`.  Built once, uploaded once.  `ids[name]` is the scan's number, `index[name]` its viewpoint -> node map.
    tables: {scan name: [n, n] float64 array in the order of scan.vpids} replaces `scan.shortest()[0]` for the scans it names (tables
    from another shortest-path code, e.g. the networkx ones the reference holds, where bit parity with that code is wanted)."""

    def __init__(self, scans, device='cuda', tables=None):
        scans = list(scans.values()) if isinstance(scans, dict) else list(scans)
        if not scans:
            raise ValueError('ScanDistances: no scans')
        self.ids = {sc.name: k for k, sc in enumerate(scans)}
        self.index = {sc.name: sc.index for sc in scans}
        blocks, off = [], [0]
        for sc in scans:
            n = len(sc.vpids)
            d = np.ascontiguousarray(tables[sc.name] if (tables and sc.name in tables) else sc.shortest()[0], np.float64)
            if d.shape != (n, n):
                raise ValueError('ScanDistances: the table of %s is %s, the scan has %d viewpoints' % (sc.name, d.shape, n))
            blocks.append(d.reshape(-1))
            off.append(off[-1] + n * n)
        self.n = np.array([len(sc.vpids) for sc in scans], np.int32)
        self.device = torch.device(device)
        self.dist = torch.from_numpy(np.concatenate(blocks)).to(self.device)
        self.off = torch.from_numpy(np.asarray(off[:-1], np.int64)).to(self.device)
        self.n_dev = torch.from_numpy(self.n).to(self.device)


def nav_metrics(sd, item_scan, pred, pred_start, ref, ref_start, goal=None, goal_start=None, margin=3.0, max_ref=None):
    """goat_nav_metrics over host index arrays (numpy; checked here against the sizes of their scans, the kernel cannot) -> float64
    [N, 12] device tensor on the current stream.  One H2D copy carries every index array."""
    N = len(item_scan)
    parts = [np.asarray(x, np.int32).reshape(-1) for x in ((item_scan, pred, pred_start, ref, ref_start) + ((goal, goal_start) if goal is not None else ()))]
    if len(parts[2]) != N + 1 or len(parts[4]) != N + 1 or (goal is not None and len(parts[6]) != N + 1):
        raise ValueError('nav_metrics: the CSR starts hold N + 1 = %d entries' % (N + 1))
    P, R = np.diff(parts[2]), np.diff(parts[4])
    if N < 1 or (P < 1).any() or (R < 1).any() or parts[2][0] != 0 or parts[4][0] != 0 or parts[2][-1] != len(parts[1]) or parts[4][-1] != len(parts[3]):
        raise ValueError('nav_metrics: every item needs at least one predicted and one reference node, and the CSR must cover its array')
    ns = sd.n[parts[0]] if (parts[0] >= 0).all() and (parts[0] < len(sd.n)).all() else None
    if ns is None:
        raise ValueError('nav_metrics: scan id outside [0, %d)' % len(sd.n))
    for nodes, cnt, what in ((parts[1], P, 'pred'), (parts[3], R, 'ref')) + (((parts[5], np.diff(parts[6]), 'goal'),) if goal is not None else ()):
        if (cnt < 0).any() or cnt.sum() != len(nodes) or (nodes < 0).any() or (nodes >= np.repeat(ns, cnt)).any():
            raise ValueError('nav_metrics: a %s node index lies outside its scan' % what)
    max_ref = int(R.max()) if max_ref is None else int(max_ref)
    if max_ref > MAX_REF or max_ref < int(R.max()):
        raise ValueError('nav_metrics: reference paths of up to %d nodes (max_ref %d; the kernel holds %d)' % (int(R.max()), max_ref, MAX_REF))
    flat = torch.from_numpy(np.concatenate(parts))
    if sd.device.type == 'cuda':
        flat = flat.pin_memory()
    flat = flat.to(sd.device, non_blocking=True)
    views, o = [], 0
    for p in parts:
        views.append(flat[o:o + len(p)])
        o += len(p)
    g, gs = (views[5], views[6]) if goal is not None else (None, None)
    if g is not None and g.numel() == 0:            # (no item has a goal node: a valid, never-read address for the non-null argument)
        g = views[6]
    out = torch.empty(N, len(COLS), dtype=torch.float64, device=sd.device)
    launch('goat_nav_metrics', sd.dist, sd.off, sd.n_dev, len(sd.n), views[0], views[1], views[2], views[3], views[4], g, gs, N, max_ref,
           float(margin), out, what='goat_nav_metrics(N=%d,max_ref=%d)' % (N, max_ref))
    return out


class NavEvaluator:
    """`eval_metrics` of the reference's environments (M/r2r/env.py:492-520; with `obj2vps`: M/reverie/env.py:555-581).

        ev = NavEvaluator(scans, gt_trajs)                       # gt_trajs: {instr_id: (scan name, gt_path)}, as R2RNavBatch.gt_trajs
        ev = NavEvaluator(scans, gt_trajs, obj2vps=obj2vps)      # {instr_id: (scan name, gt_path, gt_objid)} + {'<scan>_<objid>': [vp, ...]}
        avg_metrics, metrics = ev.eval_metrics(preds)            # preds: [{'instr_id', 'trajectory': [[vp, ...], ...], 'pred_objid'}]

    The trajectories are flattened and every viewpoint id goes through `ScanGraph.index` on the host — the only way a node index is
    formed, so an unknown id is a KeyError; an empty path or `path[0] != gt_path[0]` (the reference's assert) is a ValueError, all before
    anything touches the device.  Then one upload, one launch (goat_nav_metrics), one read-back.  Returned: the reference's keys and
    scalings (x 100 where it scales) and per-item lists, `instr_id` included; `action_steps` = len(trajectory) - 1 and `rgs` / `rgspl`
    (str(pred_objid) == str(gt_objid)) are formed on the host from the read-back.  Gathering predictions across ranks stays with the caller.
    The distance tables are uploaded at the first call.  tables: see ScanDistances."""

    def __init__(self, scans, gt_trajs, obj2vps=None, margin=3.0, device='cuda', tables=None):
        self.scans = {sc.name: sc for sc in (scans.values() if isinstance(scans, dict) else scans)}
        self.gt_trajs, self.obj2vps, self.margin = gt_trajs, obj2vps, float(margin)
        self.device, self._tables, self._sd = device, tables, None
        self._order = {name: k for k, name in enumerate(self.scans)}

    def distances(self):
        if self._sd is None:
            self._sd = ScanDistances(list(self.scans.values()), self.device, self._tables)
        return self._sd

    def _flatten(self, preds):
        """host index arrays of `preds` (validated) -> (item_scan, pred, pred_start, ref, ref_start, goal | None, goal_start | None)"""
        item_scan, pred, ref, goal = [], [], [], []
        ps, rs_, gs = [0], [0], [0]
        for item in preds:
            iid = item['instr_id']
            gt = self.gt_trajs[iid]
            scan, gt_path = gt[0], gt[1]
            ix = self.scans[scan].index
            path = [vp for hop in item['trajectory'] for vp in hop]
            if not path or not gt_path:
                raise ValueError('eval_metrics: %s has an empty %s path' % (iid, 'predicted' if not path else 'ground-truth'))
            if path[0] != gt_path[0]:
                raise ValueError('eval_metrics: %s: result trajectories should include the start position' % iid)
            pred += [ix[vp] for vp in path]
            ref += [ix[vp] for vp in gt_path]
            if self.obj2vps is not None:
                vps = self.obj2vps['%s_%s' % (scan, str(gt[2]))]
                if len(vps) == 0:
                    raise ValueError('eval_metrics: %s_%s has no goal viewpoint' % (scan, gt[2]))
                goal += [ix[vp] for vp in vps if vp in ix]           # (a viewpoint of no node of the graph can never be reached)
                gs.append(len(goal))
            item_scan.append(self._order[scan])
            ps.append(len(pred))
            rs_.append(len(ref))
        if max(b - a for a, b in zip(rs_[:-1], rs_[1:])) > MAX_REF:
            raise ValueError('eval_metrics: ground-truth paths of more than %d nodes are not supported' % MAX_REF)
        i32 = lambda x: np.asarray(x, np.int32)
        return (i32(item_scan), i32(pred), i32(ps), i32(ref), i32(rs_)) + ((i32(goal), i32(gs)) if self.obj2vps is not None else (None, None))

    def eval_metrics(self, preds):
        preds = list(preds)
        if not preds:
            raise ValueError('eval_metrics: no predictions')
        arrays = self._flatten(preds)
        cols = nav_metrics(self.distances(), *arrays, margin=self.margin).cpu().numpy()
        metrics = {'action_steps': [len(item['trajectory']) - 1 for item in preds]}
        if self.obj2vps is None:
            for c, name in enumerate(COLS):
                if name != 'gt_lengths':
                    metrics[name] = list(cols[:, c])
            metrics['instr_id'] = [item['instr_id'] for item in preds]
            avg = {'action_steps': np.mean(metrics['action_steps']), 'steps': np.mean(metrics['trajectory_steps']),
                   'lengths': np.mean(metrics['trajectory_lengths']), 'nav_error': np.mean(metrics['nav_error']),
                   'oracle_error': np.mean(metrics['oracle_error']), 'sr': np.mean(metrics['success']) * 100,
                   'oracle_sr': np.mean(metrics['oracle_success']) * 100, 'spl': np.mean(metrics['spl']) * 100,
                   'nDTW': np.mean(metrics['nDTW']) * 100, 'SDTW': np.mean(metrics['SDTW']) * 100, 'CLS': np.mean(metrics['CLS']) * 100}
            return avg, metrics
        for name in ('trajectory_steps', 'trajectory_lengths', 'success', 'oracle_success', 'spl'):
            metrics[name] = list(cols[:, COLS.index(name)])
        rgs = [str(item.get('pred_objid', None)) == str(self.gt_trajs[item['instr_id']][2]) for item in preds]
        denom = np.maximum(np.maximum(cols[:, 3], cols[:, 4]), 0.01)
        metrics['rgs'] = rgs
        metrics['rgspl'] = list(np.asarray(rgs, np.float64) * cols[:, 4] / denom)
        metrics['instr_id'] = [item['instr_id'] for item in preds]
        avg = {'action_steps': np.mean(metrics['action_steps']), 'steps': np.mean(metrics['trajectory_steps']),
               'lengths': np.mean(metrics['trajectory_lengths']), 'sr': np.mean(metrics['success']) * 100,
               'oracle_sr': np.mean(metrics['oracle_success']) * 100, 'spl': np.mean(metrics['spl']) * 100,
               'rgs': np.mean(metrics['rgs']) * 100, 'rgspl': np.mean(metrics['rgspl']) * 100}
        return avg, metrics


def validate(walk, evaluator, episode_batches, navigator=None, check_every=None):
    """The validation pass of the reference trainer (M/r2r/main_nav.py `valid`: agent.test() with argmax feedback, then
    env.eval_metrics) over captured graphs: `walk` (rollout.ArgmaxEpisode) is replayed for every batch of `episode_batches`; a batch
    shorter than the walk's B (the last one) is padded with repeats of its first episode, whose predictions are dropped.
    navigator / check_every: passed to `walk.run` (a navdev.DeviceNavigator in 'argmax' mode paces the walk on the device).
    -> (avg_metrics, metrics, preds)."""
    B = walk.B
    preds = []
    for episodes in episode_batches:
        episodes = list(episodes)
        n = len(episodes)
        if not 1 <= n <= B:
            raise ValueError('validate: a batch of %d episodes for a walk captured at B = %d' % (n, B))
        padded = episodes + [episodes[0]] * (B - n)
        traj = walk.run(padded) if (navigator is None and check_every is None) else walk.run(padded, navigator=navigator, check_every=check_every)
        for tr in traj[:n]:
            item = {'instr_id': tr['instr_id'], 'trajectory': tr['path']}
            if 'pred_objid' in tr:
                item['pred_objid'] = tr['pred_objid']
            preds.append(item)
    avg, metrics = evaluator.eval_metrics(preds)
    return avg, metrics, preds
