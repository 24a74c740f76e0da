"""The navigator of a policy-driven walk on the DEVICE (overview: rollout.py; kernels: csrc/navstate.hip).

A sampled walk (`sampled.SinglePassSampledEpisode`) and the validation walk (`sampled.ArgmaxEpisode`) are host-paced on the host
planner: per step `EpisodePlanner.build_step()` builds about twenty small tables, `EpisodeBuffers.load_part` copies them, the step
graph is replayed, the host reads the probabilities back (a synchronisation), picks the action and moves the Python navigator.  Here
the navigator's state lives in HBM and `goat_nav_step` does advance() + build_step() in two launches that write the step's tables at
the addresses the captured step graph reads: the walk is one loop of launches, without a device -> host copy or a synchronisation
before its end.  The host planner stays as it is and is the reference this module is tested against.

  * `ScanTables`        the static tables of a set of ScanGraphs (positions, candidate lists, edge lengths, shortest distances and
                        their predecessor matrices, feature rows, the view-angle table), built and uploaded once; `.host` holds them
                        as numpy arrays.
  * `DeviceNavigator`   the per-episode state block of one (B, T) bucket over an `EpisodeBuffers`, in one of three modes: 'sample'
                        (SampledEpisode.sample restated on the device), 'argmax' (the stop rule, stop scores and backtrack of the
                        validation walk) and 'forced' (a given [T, B] action tensor: TeacherEpisode.plan(actions=...)).

The DAgger labels follow `te.expert_policy`: 'spl' comes out of `goat_nav_step` itself; with 'ndtw' (the RxR scripts) a third launch per
step, `goat_nav_ndtw` (csrc/navexpert_core.hpp), writes the nDTW expert's label over it from the walked path it folds forward on the
device and the episode's ground-truth path, staged by begin() in a bucket of `max_ref` viewpoints.

A TeacherEpisode with REVERIE / SOON objects (`te.objects`) walks through `goat_nav_obj_step`, the same two launches with the object
bucket O = te.O switched on: `ObjectTables` holds the static object half (directions, boxes, categories, rows of ObjectStore.table),
`DeviceNavigator(..., objects=ObjectTables(te.objects, tables), max_end=)` writes the ten object tables of a step beside the 21 others,
begin() stages the goals (`object_goals`: end viewpoints and the target's index among their objects), and an argmax walk returns
`pred_objid` as the host planner does.

Scope: R2R-, RxR- and REVERIE-style walks.  Object walks hold at most 64 objects per viewpoint and 64 end viewpoints per episode, and
their episodes carry an explicit `obj_id` (or the simulator runs with obj_fallback=False): the stand-in target the host draws per
observation from `sim.obj_rng` cannot be restated by a kernel.  The two-pass `SampledEpisode` stays on the host planner: it needs
finish()'s joined `all_*` tables and is the slower form of the sampled half anyway."""
import time

import numpy as np
import torch

from . import _lib, layers
from ._plumbing import launch
from .nav_inputs import EXPERT_POLICIES, language_inputs
from .navsim import GraphSim, view_angle_feature_table, view_angles

MODES = {'sample': 0, 'argmax': 1, 'forced': 2}
STATUS = {1: 'the map has more nodes than the bucket of the step holds', 2: 'the panorama is wider than the bucket W',
          3: 'the action is not a selectable node of the map', 4: 'the hop log or a path stack overflowed',
          5: 'the viewpoint has more objects than the bucket obj_width'}
# the order of the address tables (csrc/navstate_core.hpp)
SCAN_TABLES = ('pos', 'cand_start', 'cand_nb', 'cand_point', 'cand_ang', 'cand_len', 'feature_row', 'vp_scan', 'scan_off', 'scan_n',
               'dist_off', 'dist', 'vaf', 'view_ang', 'pred')
OBJECT_TABLES = ('obj_start', 'obj_row', 'obj_dir', 'obj_box', 'obj_name')
# the header words of an episode's read-back block, in the order of the enum H_* of csrc/navstate_core.hpp: H[name] is the word's index
HEADER = ('cur', 'view', 'ended', 'just', 'n', 'status', 'status_t', 'start', 'goal', 'noleft', 'nscored', 'live', 'nslot', 'vlen', 'ncand',
          'startview', 'hopn', 'bt_start', 'bt_n', 'k', 'scan', 'fold', 'pred_vp', 'pred_obj', 'olen')
H = {name: i for i, name in enumerate(HEADER)}
HDR = 32
MAX_B, MAX_T, MAX_G, MAX_W, MAX_CAP, MAX_REF = 1024, 64, 256, 64, 254, 64        # GOAT_NAV_MAX_* (include/goat_hip.h)
MAX_O, MAX_END = 64, 64
_i32, _i64, _f32, _bool = torch.int32, torch.int64, torch.float32, torch.bool
# the tables of one step that the kernels write, in the order of their address tables: (name, dtype, shape) with the shape a function of
# B episodes, the step's map width G, W views and O object slots per panorama, C = A + 3 columns and n pool rows up to the step.  The
# first 21 are those of every walk (`step_tab`), the ten behind them those of an object walk (`ostep_tab`).
STEP_SPEC = (
    ('feat_idx', _i32, lambda B, G, W, O, C, n: (B * W,)), ('feat_start', _i32, lambda B, G, W, O, C, n: (B * W + 1,)),
    ('loc_fts', _f32, lambda B, G, W, O, C, n: (B, W + O, C)), ('nav_types', _i64, lambda B, G, W, O, C, n: (B, W + O)),
    ('view_lens', _i64, lambda B, G, W, O, C, n: (B,)), ('gmap_step_ids', _i64, lambda B, G, W, O, C, n: (B, G)),
    ('gmap_pos_fts', _f32, lambda B, G, W, O, C, n: (B, G, C)), ('gmap_pair_dists', _f32, lambda B, G, W, O, C, n: (B, G, G)),
    ('gmap_visited_masks', _bool, lambda B, G, W, O, C, n: (B, G)), ('gmap_masks', _bool, lambda B, G, W, O, C, n: (B, G)),
    ('vp_pos_fts', _f32, lambda B, G, W, O, C, n: (B, W + O + 2, 2 * C)), ('vp_masks', _bool, lambda B, G, W, O, C, n: (B, W + O + 2)),
    ('vp_nav_masks', _bool, lambda B, G, W, O, C, n: (B, W + O + 2)), ('nav_fusion', _f32, lambda B, G, W, O, C, n: (B, G, W + O + 2)),
    ('target', _i64, lambda B, G, W, O, C, n: (B,)), ('csr_idx', _i32, lambda B, G, W, O, C, n: (n,)),
    ('csr_start', _i32, lambda B, G, W, O, C, n: (B * G + 1,)), ('csr_scale', _f32, lambda B, G, W, O, C, n: (B * G,)),
    ('inv_idx', _i32, lambda B, G, W, O, C, n: (n,)), ('inv_start', _i32, lambda B, G, W, O, C, n: (n + 1,)),
    ('inv_w', _f32, lambda B, G, W, O, C, n: (n,)),
    ('obj_idx', _i32, lambda B, G, W, O, C, n: (B * O,)), ('obj_start', _i32, lambda B, G, W, O, C, n: (B * O + 1,)),
    ('reverie_obj_lens', _i64, lambda B, G, W, O, C, n: (B,)), ('reverie_obj_names', _i64, lambda B, G, W, O, C, n: (B, O)),
    ('vp_obj_masks', _bool, lambda B, G, W, O, C, n: (B, W + O + 2)), ('obj_target', _i64, lambda B, G, W, O, C, n: (B,)),
    ('ocat_idx', _i32, lambda B, G, W, O, C, n: (B * (W + O),)), ('ocat_start', _i32, lambda B, G, W, O, C, n: (B * (W + O) + 1,)),
    ('ocat_inv_idx', _i32, lambda B, G, W, O, C, n: (B * (W + O),)), ('ocat_inv_start', _i32, lambda B, G, W, O, C, n: (B * W + B * O + 1,)))
N_STEP = 21
STEP_TABLES = tuple((name, dtype) for name, dtype, _ in STEP_SPEC[:N_STEP])
OBJECT_STEP_TABLES = tuple((name, dtype) for name, dtype, _ in STEP_SPEC[N_STEP:])


def workspace(B, T, W, O=0):
    """the tail's workspace as `Workspace` of csrc/navstate_core.hpp lays it out -> (its size in ints, the index of the live count)"""
    live_at = 2 * (B + 1) + T * (B * (W + O) + B) + B
    return live_at + 1 + (B + 1 if O else 0), live_at


class _Staging:
    """What begin() hands to the device in one copy: `fields` [(name, torch dtype, shape)] laid out one behind the other in a pinned host
    buffer and its device twin.  host[name] / dev[name]: the numpy / device views of a field."""

    def __init__(self, fields, device):
        at, n = {}, 0
        for name, dtype, shape in fields:
            at[name] = (n, n + int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size())
            n = at[name][1]
        self.pinned = torch.zeros(n, dtype=torch.uint8)
        if device.type == 'cuda':
            self.pinned = self.pinned.pin_memory()
        self.device = torch.zeros(n, dtype=torch.uint8, device=device)
        self.host = {name: self.pinned[slice(*at[name])].view(dtype).view(shape).numpy() for name, dtype, shape in fields}
        self.dev = {name: self.device[slice(*at[name])].view(dtype).view(shape) for name, dtype, shape in fields}

    def upload(self):
        self.device.copy_(self.pinned, non_blocking=True)


def _pack(host, names, device):
    """one packed buffer, one H2D copy -> (the buffer, the addresses of the tables inside it as a device int64 tensor)"""
    offs, n = [], 0
    for name in names:
        offs.append(n)
        n += (max(host[name].nbytes, 1) + 15) // 16 * 16
    flat = torch.zeros(n, dtype=torch.uint8)
    for name, o in zip(names, offs):
        raw = np.ascontiguousarray(host[name]).view(np.uint8).reshape(-1)
        flat[o:o + raw.size] = torch.from_numpy(raw)
    if device.type == 'cuda':
        flat = flat.pin_memory()
    dev = flat.to(device, non_blocking=True)
    base = dev.data_ptr()
    return dev, torch.tensor([base + o for o in offs], dtype=torch.int64).to(device)


class ScanTables:
    """The read-only tables `goat_nav_step` walks on, for the ScanGraphs `scans`.  Viewpoints are numbered across the scans
    (`first[scan name]` + the scan's own index); per viewpoint: position, the candidate list in the order of `ScanGraph.candidates(vp)`
    (neighbour, pointId, normalized heading / elevation, and the edge length exactly as `GraphMap.update_graph` computes it) and the
    feature row; per scan: the all-pairs distances of `ScanGraph.shortest()` and, at the same offsets, its predecessor matrix (`pred`,
    int32, scan-local indices: `pred[i, j]` comes before j on the shortest path from i).  row_of: `row(scan_name, vp) -> int` or an object with that
    method (features.FeatureStore).  device=None keeps the tables on the host only (`.host`: {name: numpy array})."""

    def __init__(self, scans, row_of, angle_feat_size=4, device='cuda'):
        scans = list(scans.values() if isinstance(scans, dict) else scans)
        row = row_of.row if hasattr(row_of, 'row') else row_of
        self.scans, self.A = scans, angle_feat_size
        self.ids = {sc.name: k for k, sc in enumerate(scans)}
        self.first, self.names = {}, []
        for sc in scans:
            self.first[sc.name] = len(self.names)
            self.names += list(sc.vpids)
        pos, cstart, cnb, cpt, cang, clen, frow, vscan, dist, doff, pred = [], [0], [], [], [], [], [], [], [], [0], []
        for k, sc in enumerate(scans):
            off = self.first[sc.name]
            for vp in sc.vpids:
                p = np.asarray(tuple(float(x) for x in sc.pos[sc.index[vp]]), np.float64)
                for c in sc.candidates(vp):
                    d = np.asarray(c['position'], np.float64) - p
                    clen.append(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))             # navsim.GraphMap.update_graph
                    cnb.append(off + sc.index[c['viewpointId']])
                    cpt.append(c['pointId'])
                    cang.append((c['normalized_heading'], c['normalized_elevation']))
                cstart.append(len(cnb))
                frow.append(row(sc.name, vp))
                vscan.append(k)
            pos.append(sc.pos)
            dist.append(np.asarray(sc.shortest()[0], np.float64).reshape(-1))
            pred.append(np.asarray(sc.shortest()[1], np.int32).reshape(-1))
            doff.append(doff[-1] + dist[-1].size)
        self.host = {
            'pos': np.concatenate(pos, 0).astype(np.float64), 'cand_start': np.asarray(cstart, np.int32), 'cand_nb': np.asarray(cnb, np.int32),
            'cand_point': np.asarray(cpt, np.int32), 'cand_ang': np.asarray(cang, np.float64).reshape(-1, 2), 'cand_len': np.asarray(clen, np.float64),
            'feature_row': np.asarray(frow, np.int32), 'vp_scan': np.asarray(vscan, np.int32),
            'scan_off': np.asarray([self.first[sc.name] for sc in scans], np.int32), 'scan_n': np.asarray([len(sc.vpids) for sc in scans], np.int32),
            'dist_off': np.asarray(doff[:-1], np.int64), 'dist': np.concatenate(dist), 'vaf': view_angle_feature_table(angle_feat_size),
            'view_ang': np.asarray([view_angles(v) for v in range(36)], np.float64), 'pred': np.concatenate(pred)}
        self.device = None if device is None else torch.device(device)
        self.dev, self.tab = None, None
        if self.device is not None:
            self._upload()

    def vp(self, scan_name, vpid):
        """the number of a viewpoint in these tables"""
        sc = self.scans[self.ids[scan_name]]
        return self.first[scan_name] + sc.index[vpid]

    def _upload(self):
        """one packed buffer, one H2D copy; `tab` = the addresses of the tables inside it (device int64 [15])"""
        self.dev, self.tab = _pack(self.host, SCAN_TABLES, self.device)


class ObjectTables:
    """The static object half of REVERIE / SOON observations for `goat_nav_obj_step`, as ScanTables holds the view half: indexed by the
    viewpoint numbers of `tables` (a ScanTables).  objects: an ObjectStore or its `.meta()` (no feature table is read).  Per viewpoint
    `obj_start` int32 [V + 1] (CSR over the objects below) and `obj_row` int32 [V], the viewpoint's first row in ObjectStore.table (its
    rows are contiguous: `attributes` returns an arange); per object `obj_dir` float64 [N, 2] (the stored directions), `obj_box` float32
    [N, 3] formed as `ObjectStore.attributes` forms them (h / 480 and w / 640 rounded to float32, their float32 product: independent of the
    heading) and `obj_name` int64 [N].  `ids[v]`: the object ids of viewpoint v on the host (for `pred_objid`).  device=None keeps the
    tables on the host only (`.host`)."""

    def __init__(self, objects, tables, device='cuda'):
        self.tables = tables
        start, row, dirs, box, name, self.ids = [0], [], [], [], [], []
        for sc in tables.scans:
            for vp in sc.vpids:
                k = '%s_%s' % (sc.name, vp)
                o, a = objects.count.get(k, 0), objects.attrs.get(k)
                row.append(objects.start.get(k, 0))
                self.ids.append(list(a['obj_ids'])[:o] if o else [])
                if o:
                    b = np.zeros((o, 3), np.float32)
                    b[:, 0], b[:, 1] = a['sizes'][:o, 1] / 480, a['sizes'][:o, 0] / 640
                    b[:, 2] = b[:, 0] * b[:, 1]
                    dirs.append(np.asarray(a['directions'][:o], np.float64))
                    box.append(b)
                    name.append(np.asarray(a['names'][:o], np.int64))
                start.append(start[-1] + o)
        self.host = {'obj_start': np.asarray(start, np.int32), 'obj_row': np.asarray(row, np.int32),
                     'obj_dir': np.concatenate(dirs, 0) if dirs else np.zeros((0, 2), np.float64),
                     'obj_box': np.concatenate(box, 0) if box else np.zeros((0, 3), np.float32),
                     'obj_name': np.concatenate(name) if name else np.zeros(0, np.int64)}
        self.device = None if device is None else torch.device(device)
        self.dev, self.tab = None, None
        if self.device is not None:
            self.dev, self.tab = _pack(self.host, OBJECT_TABLES, self.device)


def object_goals(episodes, objtables, max_end, obj_fallback=False):
    """The goals of object walks as `goat_nav_obj_step` reads them -> int32 [B, max_end, 2]: per episode its `end_vps` as viewpoint
    numbers (-1: unused pair) and, per end viewpoint, the index of the target among that viewpoint's objects by the reference's
    `str(oid) == str(gt_obj_id)` rule (nav_inputs.teacher_object: the first match), or -1 (absent, or `obj_id` None).
    obj_fallback (te.sim.obj_fallback): the host then draws a stand-in target from `sim.obj_rng` per observation for an episode without
    `obj_id`, a sequence no kernel can restate: such an episode raises ValueError here."""
    goals = np.full((len(episodes), max_end, 2), -1, np.int32)
    tables = objtables.tables
    for i, e in enumerate(episodes):
        ends = list(e.get('end_vps') or [])
        if len(ends) > max_end:
            raise ValueError('DeviceNavigator: episode %d has %d end viewpoints, the bucket max_end holds %d' % (i, len(ends), max_end))
        if e.get('obj_id') is None and obj_fallback:
            raise ValueError('DeviceNavigator: episode %d has no obj_id and the simulator draws a random stand-in target per observation '
                             '(GraphSim(obj_fallback=True)); the device navigator needs explicit targets or obj_fallback=False' % i)
        for k, vp in enumerate(ends):
            v = tables.vp(e['scan'].name, vp)
            goals[i, k, 0] = v
            for j, oid in enumerate(objtables.ids[v]):
                if str(oid) == str(e.get('obj_id')):
                    goals[i, k, 1] = j
                    break
    return goals


class DeviceNavigator:
    """The navigator state of B episodes of the bucket (T steps, panorama width W, map widths te.gw) over the tensors of `bufs`.

        tables = ScanTables(scans, store);  nav = DeviceNavigator(te, tables, bufs, 'sample')
        traj, actions = sp.run(episodes, rng, navigator=nav)                 # SinglePassSampledEpisode / ArgmaxEpisode

    By hand: begin(episodes, rng | actions) -> for t in 0..T-1: step(t, act) then the step graph -> step(T, act) -> finish().
    max_ref (te.expert_policy = 'ndtw' only): the bucket of the ground-truth path in viewpoints, at most 64; begin() raises ValueError
    for a longer path, before any launch.
    objects (required when te.objects is set): the ObjectTables of te.objects over the same `tables`; max_end: the bucket of an episode's
    `end_vps`, at most 64 (begin() raises ValueError for a longer list).  finish() of an argmax walk then adds 'pred_objid' to every
    trajectory (the id, or None for a viewpoint without objects or a walk that scored no node).
    begin() is one pinned H2D copy (scan, start viewpoint and view, goal per episode; the uniforms `rng.random_sample((T, B))`, the
    numbers the host walk draws step by step, in its order; the forced actions; the ground-truth paths for the nDTW expert) next to the instruction's `txt_ids` / `txt_masks`;
    step() launches the kernels and recomputes, into the same storage and in stream order, the memoised masks derived from the step's
    tables (a raw kernel write does not bump a tensor's version counter); finish() is the one read-back: status words, actions, hop log
    and n_traj.  A non-zero status word is raised there as a ValueError naming episode and step.  Nothing in between synchronises."""

    def __init__(self, te, tables, bufs, mode, max_ref=32, objects=None, max_end=32):
        if te.objects is not None and objects is None:
            raise NotImplementedError('DeviceNavigator: a walk with REVERIE / SOON objects needs their device tables: pass '
                                      'objects=ObjectTables(te.objects, tables)')
        if objects is not None and te.objects is None:
            raise ValueError('DeviceNavigator: object tables for a TeacherEpisode without objects')
        if mode not in MODES:
            raise ValueError('DeviceNavigator: mode is one of %s, got %r' % (sorted(MODES), mode))
        self.expert = getattr(te, 'expert_policy', 'spl')
        if self.expert not in EXPERT_POLICIES:
            raise ValueError('DeviceNavigator: expert_policy is one of %s, got %r' % (EXPERT_POLICIES, self.expert))
        if self.expert == 'ndtw' and not 1 <= max_ref <= MAX_REF:
            raise ValueError('DeviceNavigator: max_ref = %d outside what goat_nav_ndtw holds (1..%d)' % (max_ref, MAX_REF))
        self.max_ref = max_ref
        if tables.A != te.sim.angle_feat_size:
            raise ValueError('DeviceNavigator: the scan tables hold %d angle features, the simulator %d' % (tables.A, te.sim.angle_feat_size))
        self.te, self.tables, self.bufs, self.mode = te, tables, bufs, mode
        self.device = bufs.device
        t_ = bufs.t
        self.B, self.T, self.W, self.A = t_['txt_ids'].shape[0], te.T, te.W, tables.A
        B, T, W = self.B, self.T, self.W
        self.gw = [int(te.gw(t)) for t in range(T)]
        self.cap = max(self.gw) - 2
        if not (1 <= B <= MAX_B and 1 <= T <= MAX_T and 36 <= W <= MAX_W and 1 <= self.cap <= MAX_CAP and max(self.gw) <= MAX_G and min(self.gw) >= 2):
            raise ValueError('DeviceNavigator: B = %d, T = %d, W = %d, map widths %d..%d outside what goat_nav_step holds (B <= %d, T <= %d, '
                             '36 <= W <= %d, width <= %d)' % (B, T, W, min(self.gw), max(self.gw), MAX_B, MAX_T, MAX_W, min(MAX_G, MAX_CAP + 2)))
        # object walks: O object slots behind the W views of every panorama, goals in a bucket of max_end end viewpoints
        self.objects, self.max_end = objects, max_end
        self.O = O = int(te.O) if objects is not None else 0
        if objects is not None:
            if objects.tables is not tables:
                raise ValueError('DeviceNavigator: the object tables are numbered by another ScanTables')
            if self.expert != 'spl':
                raise ValueError('DeviceNavigator: the REVERIE / SOON agent has the shortest-path expert only')
            if not (1 <= O <= MAX_O and 1 <= max_end <= MAX_END):
                raise ValueError('DeviceNavigator: obj_width = %d, max_end = %d outside what goat_nav_obj_step holds (1..%d, 1..%d)'
                                 % (O, max_end, MAX_O, MAX_END))
        WT = self.WT = W + O
        self._step_tensors = []
        ptrs, optrs = [], []
        for t in range(T):
            n = (t + 1) * (B * WT + B) + (B if t > 0 else 0)
            ts = []
            for name, dtype, shape in STEP_SPEC if O else STEP_SPEC[:N_STEP]:
                v, want = t_.get('s%d_%s' % (t, name)), shape(B, self.gw[t], W, O, self.A + 3, n)
                if v is None or tuple(v.shape) != want or v.dtype != dtype:
                    raise ValueError('DeviceNavigator: s%d_%s is %s, the navigator writes %s %s' % (
                        t, name, None if v is None else (tuple(v.shape), v.dtype), want, dtype))
                ts.append(v)
            self._step_tensors.append(ts)
            ptrs.append([v.data_ptr() for v in ts[:N_STEP]])
            optrs.append([v.data_ptr() for v in ts[N_STEP:]])
        h = _lib.lib()
        self.state_ints = h.goat_nav_obj_state_ints(T, W, O, self.cap) if O else h.goat_nav_state_ints(T, W, self.cap)
        self.log_ints = h.goat_nav_log_ints(T, self.cap)
        if self.state_ints <= 0 or self.log_ints <= 0:
            raise RuntimeError('libgoat_hip: goat_nav_state_ints(T=%d, W=%d, O=%d, cap=%d) gave no size' % (T, W, O, self.cap))
        dev = self.device
        self.step_tab = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        self.ostep_tab = torch.tensor(optrs, dtype=torch.int64).to(dev) if O else None
        self.si = torch.zeros(B * self.state_ints, dtype=torch.int32, device=dev)
        self.sd = torch.zeros(B * (self.cap * self.cap + self.cap), dtype=torch.float64, device=dev)
        self.log = torch.zeros(2 * T * B + B * self.log_ints, dtype=torch.int32, device=dev)
        ws_ints, self._live_at = workspace(B, T, W, O)
        self.ws = torch.zeros(ws_ints, dtype=torch.int32, device=dev)
        # staging of begin(): the uniforms, (scan, start viewpoint, start view, goal) per episode, the forced actions; for the nDTW
        # expert the ground-truth paths (length, viewpoint numbers) and for an object walk the goals behind them
        ndtw = self.expert == 'ndtw'
        self._stage = _Staging([('u', torch.float64, (T, B)), ('ep', _i32, (B, 4)), ('forced', _i32, (T, B))]
                               + ([('ref', _i32, (B, max_ref + 1))] if ndtw else []) + ([('goal', _i32, (B, max_end, 2))] if O else []), dev)
        d = self._stage.dev
        self.u, self.ep, self.forced, self.ref, self.goal = d['u'], d['ep'], d['forced'], d.get('ref'), d.get('goal')
        self._log_host = torch.zeros(self.log.numel(), dtype=torch.int32)
        if dev.type == 'cuda':
            self._log_host = self._log_host.pin_memory()
        self._copied = None
        self.episodes = None
        self.launches_per_step = 2
        if ndtw:
            # the DTW row of the walked path and one working row per map node: sized by this navigator's cap and max_ref, not by the
            # limits of the ABI (there: 133 KB per episode)
            self.expert_doubles = h.goat_nav_expert_doubles(self.cap, max_ref)
            if self.expert_doubles <= 0:
                raise RuntimeError('libgoat_hip: goat_nav_expert_doubles(cap=%d, max_ref=%d) gave no size' % (self.cap, max_ref))
            self.xd = torch.zeros(B * self.expert_doubles, dtype=torch.float64, device=dev)
            self.launches_per_step = 3

    # ---- one walk -------------------------------------------------------------------------------------------------------------
    def begin(self, episodes, rng=None, actions=None, text='host'):
        """start_walk for `episodes` ({instr_id, scan (ScanGraph), path, heading, instr_encoding}).  'sample': rng (numpy RandomState)
        gives the uniforms; 'forced': actions [<= T, B] integers (missing steps are [stop], as TeacherEpisode.plan pads them).
        text='device': the instruction is what a kernel wrote into bufs.t['txt_ids'] / bufs.t['txt_masks'] already
        (speaker.BackTranslator.run): nothing is packed or uploaded for it and `instr_encoding` is not read."""
        if text not in ('host', 'device'):
            raise ValueError("DeviceNavigator: text is 'host' or 'device', got %r" % (text,))
        te, B, T = self.te, self.B, self.T
        if len(episodes) != B:
            raise ValueError('DeviceNavigator: %d episodes for a state block of B = %d' % (len(episodes), B))
        t0 = time.perf_counter()
        if self._copied is not None:
            self._copied.synchronize()              # the previous H2D has read the pinned buffer
        st = self._stage.host
        u, ep, forced = st['u'], st['ep'], st['forced']
        if self.mode == 'sample':
            u[:] = (rng if rng is not None else np.random.RandomState(0)).random_sample((T, B))
        forced[:] = 0
        if self.mode == 'forced':
            if actions is None:
                raise ValueError('DeviceNavigator: a forced walk needs its actions')
            acts = np.asarray([np.asarray(a, np.int64) for a in actions], np.int64).reshape(-1, B)
            if len(acts) > T:
                raise ValueError('%d recorded steps exceed the episode bucket T = %d' % (len(acts), T))
            forced[:len(acts)] = acts
        if self.expert == 'ndtw':
            ref = st['ref']
            for i, e in enumerate(episodes):
                if not 1 <= len(e['path']) <= self.max_ref:
                    raise ValueError('DeviceNavigator: the ground-truth path of episode %d has %d viewpoints, the bucket max_ref holds 1..%d'
                                     % (i, len(e['path']), self.max_ref))
            ref[:] = 0
            for i, e in enumerate(episodes):
                ref[i, 0] = len(e['path'])
                ref[i, 1:1 + len(e['path'])] = [self.tables.vp(e['scan'].name, vp) for vp in e['path']]
        if self.O:
            st['goal'][:] = object_goals(episodes, self.objects, self.max_end, bool(getattr(te.sim, 'obj_fallback', False)))
        for i, e in enumerate(episodes):
            name = e['scan'].name
            ep[i] = (self.tables.ids[name], self.tables.vp(name, e['path'][0]), GraphSim._snap(e['heading'], 0.0), self.tables.vp(name, e['path'][-1]))
        if text == 'host':
            lang = language_inputs([{'instr_encoding': e['instr_encoding']} for e in episodes])
            n = lang['txt_ids'].shape[1]
            if n > te.L:
                raise ValueError('instruction of %d tokens exceeds the text bucket %d' % (n, te.L))
            ids = torch.zeros(B, te.L, dtype=torch.int64)
            msk = torch.zeros(B, te.L, dtype=torch.bool)
            ids[:, :n], msk[:, :n] = lang['txt_ids'], lang['txt_masks']
            self.bufs.load_part({'txt_ids': ids, 'txt_masks': msk})
        self._stage.upload()
        if self.device.type == 'cuda':
            self._copied = torch.cuda.Event()
            self._copied.record()
        self.episodes = list(episodes)
        self.host_s = time.perf_counter() - t0          # seconds of host work of this walk (packing here, the trajectories in finish())
        if self.O:
            launch('goat_nav_obj_reset', self.tables.tab, self.si, self.sd, self.log, self.ep, B, T, self.W, self.O, self.cap,
                   what='goat_nav_obj_reset(B=%d,T=%d,O=%d,cap=%d)' % (B, T, self.O, self.cap))
            return
        launch('goat_nav_reset', self.tables.tab, self.si, self.sd, self.log, self.ep, B, T, self.W, self.cap,
               what='goat_nav_reset(B=%d,T=%d,cap=%d)' % (B, T, self.cap))

    def step(self, t, act=None):
        """the move of step t - 1 decided from `act` (the step's probabilities [B, G] in 'sample' mode, the [3, B] argmax tensor of
        the step graph in 'argmax' mode; 'forced' reads its own tensor), then the tables of step t (none at t == T)."""
        B, T = self.B, self.T
        if self.mode == 'forced':
            act = self.forced
        if t > 0 and act is None:
            raise ValueError('DeviceNavigator.step(%d): the %s walk decides from the outputs of step %d' % (t, self.mode, t - 1))
        if self.O:
            launch('goat_nav_obj_step', self.tables.tab, self.objects.tab, self.step_tab[t] if t < T else None,
                   self.ostep_tab[t] if t < T else None, self.si, self.sd, self.log, self.ws, act if t > 0 else None, self.u, self.goal,
                   MODES[self.mode], t, B, T, self.gw[t - 1] if t > 0 else 0, self.gw[t] if t < T else 0, self.W, self.O, self.max_end,
                   self.A, self.cap, int(self.te.ignoreid), what='goat_nav_obj_step(t=%d,B=%d)' % (t, B))
        else:
            launch('goat_nav_step', self.tables.tab, self.step_tab[t] if t < T else None, self.si, self.sd, self.log, self.ws,
                   act if t > 0 else None, self.u, MODES[self.mode], t, B, T, self.gw[t - 1] if t > 0 else 0, self.gw[t] if t < T else 0,
                   self.W, self.A, self.cap, int(self.te.ignoreid), what='goat_nav_step(t=%d,B=%d)' % (t, B))
        if t < T and self.expert == 'ndtw':
            launch('goat_nav_ndtw', self.tables.tab, self.step_tab[t], self.si, self.sd, self.log, self.ref, self.xd, t, B, T, self.W, self.cap,
                   self.max_ref, int(self.te.ignoreid), what='goat_nav_ndtw(t=%d,B=%d)' % (t, B))
        if t < T:
            layers.refresh_masks(only=self._step_tensors[t], force=True)

    def finish(self):
        """the read-back of the walk -> (traj, actions [steps][B], n_traj, ended [B]); raises ValueError on a status word."""
        B, T = self.B, self.T
        self._log_host.copy_(self.log, non_blocking=True)
        if self.device.type == 'cuda':
            torch.cuda.current_stream().synchronize()
        t0 = time.perf_counter()
        log = self._log_host.numpy()
        acts, alive = log[:T * B].reshape(T, B), log[T * B:2 * T * B].reshape(T, B)
        blocks = log[2 * T * B:].reshape(B, self.log_ints)
        for i in range(B):
            if blocks[i, H['status']]:
                raise ValueError('device navigator: episode %d, step %d: %s' % (i, int(blocks[i, H['status_t']]), STATUS.get(int(blocks[i, H['status']]), 'status %d' % blocks[i, H['status']])))
        names = self.tables.names
        traj = []
        for i, e in enumerate(self.episodes):
            hs, hops = blocks[i, HDR:HDR + T + 2], blocks[i, HDR + T + 2:]
            path = [[e['path'][0]]]
            for t in range(T):
                if hs[t + 1] > hs[t]:
                    path.append([names[v] for v in hops[hs[t]:hs[t + 1]]])
            if blocks[i, H['bt_n']]:
                s = int(blocks[i, H['bt_start']])
                path.append([names[v] for v in hops[s:s + int(blocks[i, H['bt_n']])]])
            traj.append({'instr_id': e['instr_id'], 'path': path})
            if self.O and self.mode == 'argmax':        # EpisodePlanner(feedback='argmax'): the best object of the best stop node
                v, j = int(blocks[i, H['pred_vp']]) - 1, int(blocks[i, H['pred_obj']])
                traj[-1]['pred_objid'] = self.objects.ids[v][j] if (v >= 0 and j >= 0) else None
        actions = [acts[t].astype(np.int64) for t in range(T) if alive[t].any()]
        self.alive = alive.astype(bool)
        self.host_s += time.perf_counter() - t0
        return traj, actions, int(blocks[:, H['live']].sum()), blocks[:, H['ended']].astype(bool)

    def walk(self, ep, episodes, rng=None, actions=None, act=None, after=None, check_every=None, text='host'):
        """the whole walk over the graphs of `ep` (g_lang, g_step): begin, per step the navigator then the step graph, the last move,
        `after()` (the backward graph of the single pass), the read-back.  act(t): the tensor step t + 1 decides from.
        check_every=k: before every k-th step graph the host reads the number of episodes still walking (one int; this synchronises) and
        leaves the loop at zero, as speaker.IncrementalDecoder does — for walks that end long before T and whose later step graphs
        nobody needs (the validation walk; not the single pass, whose backward graph differentiates through every step).
        text: as begin()."""
        self.begin(episodes, rng, actions, text)
        ep.g_lang.replay()
        done = False
        for t in range(self.T):
            self.step(t, act(t - 1) if (t > 0 and act is not None) else None)
            if check_every and t > 0 and t % check_every == 0 and int(self.ws[self._live_at].item()) == 0:
                done = True
                break
            ep.g_step[t].replay()
        if not done:
            self.step(self.T, act(self.T - 1) if act is not None else None)
        if after is not None:
            after()
        return self.finish()
