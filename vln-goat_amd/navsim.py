"""The graph-only navigator and the maps of the fine-tuning rollout (overview, and what M/ stands for: rollout.py).  The bottom
layer: numpy, torch tensors and `features` only; nothing here imports nav_inputs.py, rollout.py, episodes.py or sampled.py.

  * `ScanGraph` / `GraphSim`      the graph-only navigator: connectivity JSON (or a synthetic scan) -> positions, adjacency,
                                  per-viewpoint candidate tables (M/r2r/env.py:241-333 `make_candidate` without the simulator),
                                  observations of `_get_obs` (:335-377), teleport steps of `make_equiv_action` (M/r2r/agent.py:349-378).
  * `FloydGraph` / `GraphMap`     the reference's map with the SAME update rule (single-pivot relaxation per visited node, the
                                  95959595 default distance, lazily evaluated `_point` paths) as vectorised float64 numpy — decisions
                                  are bit-identical to the reference's Python floats (tests/golden/rollout_walk.npz).
  * `NodeEmbedStore`              the node-embedding half of GraphMap on the DEVICE: panorama outputs of every step stay in HBM as a
                                  pool; "rewrite" / "sum + count" / "mean on read" (graph_utils.py:113-125) become a CSR gather /
                                  segment-mean over that pool (goat_gather_segmean_*), differentiable, so the gradient of a later
                                  step's map tokens reaches the panorama encoder of the step that produced them — as it does in the
                                  reference through `pad_tensors_wgrad` (M/r2r/agent.py:211).

MatterSim itself is absent from this image: the candidate ORDER inside a panorama (first view index in which a neighbour falls
inside the camera frustum, then angular distance) restates the simulator's documented behaviour and is pinned by this repo's own
fixtures only; everything downstream of the observations is pinned to outputs of the imported reference
(tests/golden/make_golden_rollout.py)."""
import json
import math
import os

import numpy as np
import torch

MAX_DIST = 30          # M/models/graph_utils.py:4-5
MAX_STEP = 10
FLOYD_INF = 95959595   # graph_utils.py:45 (the reference's "not connected" distance; also the never-written diagonal)
HFOV = math.radians(80.0)      # 640 x 480 at VFOV 60 (M/r2r/env.py:41-44)
VFOV = math.radians(60.0)


# ------------------------------------------------------------------------------------------------ geometry (M/utils/data.py)
def angle_feature(heading, elevation, angle_feat_size=4):
    # M/utils/data.py:128-131
    return np.array([math.sin(heading), math.cos(heading), math.sin(elevation), math.cos(elevation)] * (angle_feat_size // 4), dtype=np.float32)


def get_angle_fts(headings, elevations, angle_feat_size=4):
    # M/utils/data.py:177-183 (sin / cos of the float32 angles)
    headings, elevations = np.asarray(headings), np.asarray(elevations)
    ang = np.empty((headings.shape[0], 4), np.float32)
    ang[:, 0], ang[:, 1], ang[:, 2], ang[:, 3] = np.sin(headings), np.cos(headings), np.sin(elevations), np.cos(elevations)
    reps = angle_feat_size // 4
    return np.concatenate([ang] * reps, 1) if reps > 1 else ang


def view_angles(view_index):
    """heading, elevation of discretised view 0..35 (12 headings x 3 elevations, M/r2r/env.py:71-74)."""
    return (view_index % 12) * math.radians(30), (view_index // 12 - 1) * math.radians(30)


def view_angle_feature_table(angle_feat_size=4):
    """[36 base views][36 views, angle_feat_size]: get_all_point_angle_feature (M/utils/data.py:133-156) — the simulator is only
    used there to enumerate the 36 (heading, elevation) pairs."""
    out = np.empty((36, 36, angle_feat_size), np.float32)
    for base in range(36):
        bh, be = view_angles(base)
        for ix in range(36):
            h, e = view_angles(ix)
            out[base, ix] = angle_feature(h - bh, e - be, angle_feat_size)
    return out


def rel_pos(a, b):
    """absolute heading / elevation / distance of points b [n,3] seen from a [3] (calculate_vp_rel_pos_fts, M/utils/data.py:158-175,
    before the base angles are subtracted), float64."""
    b = np.asarray(b, np.float64).reshape(-1, 3)
    a = np.asarray(a, np.float64)
    dx, dy, dz = b[:, 0] - a[0], b[:, 1] - a[1], b[:, 2] - a[2]
    xy = np.maximum(np.sqrt(dx ** 2 + dy ** 2), 1e-8)
    xyz = np.maximum(np.sqrt(dx ** 2 + dy ** 2 + dz ** 2), 1e-8)
    heading = np.arcsin(dx / xy)
    heading = np.where(b[:, 1] < a[1], np.pi - heading, heading)
    elevation = np.arcsin(dz / xyz)
    return heading, elevation, xyz


# ------------------------------------------------------------------------------------------------ the map (graph_utils.py)
class FloydGraph:
    """M/models/graph_utils.py:43-88 on dense float64 matrices.  `update(k)` is the reference's single-pivot relaxation: inside
    its double loop only entries [x][k] and [k][y] are read and neither can improve (the diagonal keeps the 95959595 default), so
    the loop is order-independent and one vectorised min; `_point` is kept as an index matrix and paths are expanded lazily from
    its CURRENT state, exactly as `path()` recurses in the reference."""

    def __init__(self, cap=32):
        self.ids, self.names = {}, []
        self.D = np.full((cap, cap), float(FLOYD_INF))
        self.P = np.full((cap, cap), -1, np.int32)
        self._visited = set()
        self._hop_memo = {}         # (i, j) -> hops under the CURRENT _point matrix (cleared whenever an entry of P changes)

    def _ix(self, vp):
        i = self.ids.get(vp)
        if i is None:
            i = self.ids[vp] = len(self.names)
            self.names.append(vp)
            if i >= self.D.shape[0]:
                cap = 2 * self.D.shape[0]
                D = np.full((cap, cap), float(FLOYD_INF))
                P = np.full((cap, cap), -1, np.int32)
                D[:i, :i], P[:i, :i] = self.D[:i, :i], self.P[:i, :i]
                self.D, self.P = D, P
        return i

    def distance(self, x, y):
        if x == y:
            return 0
        return self.D[self._ix(x), self._ix(y)]

    def add_edge(self, x, y, dis):
        i, j = self._ix(x), self._ix(y)
        if dis < self.D[i, j]:
            self.D[i, j] = self.D[j, i] = dis
            self.P[i, j] = self.P[j, i] = -1
            self._hop_memo.clear()

    def update(self, k):
        kk, n = self._ix(k), len(self.names)
        D, P = self.D[:n, :n], self.P[:n, :n]
        cand = D[:, kk][:, None] + D[kk, :][None, :]
        better = cand < D
        np.fill_diagonal(better, False)
        D[better] = cand[better]
        P[better] = kk
        self._hop_memo.clear()
        self._visited.add(k)

    def visited(self, k):
        return k in self._visited

    def _hops(self, i, j, depth=0):
        if i == j:
            return 0
        memo = self._hop_memo
        n = memo.get((i, j))
        if n is None:               # (sub-paths are shared between the pairs a step asks for)
            k = int(self.P[i, j])
            if k < 0:
                n = 1
            else:
                if depth > 4096:
                    raise RecursionError('FloydGraph: cyclic _point chain')
                n = self._hops(i, k, depth + 1) + self._hops(k, j, depth + 1)
            memo[(i, j)] = n
        return n

    def path_len(self, x, y):
        return self._hops(self._ix(x), self._ix(y))

    def path(self, x, y):
        if x == y:
            return []
        i, j = self._ix(x), self._ix(y)
        k = self.P[i, j]
        if k < 0:
            return [y]
        return self.path(x, self.names[k]) + self.path(self.names[k], y)

    def dist_rows(self, x, ys):
        """distance(x, y) for every y of ys (vectorised read; 0 where y == x)."""
        i = self._ix(x)
        j = np.array([self._ix(y) for y in ys], dtype=np.int64)
        d = self.D[i, j].copy()
        d[j == i] = 0
        return d


class GraphMap:
    """M/models/graph_utils.py:91-144 without the embeddings (those live on the device: NodeEmbedStore)."""

    def __init__(self, start_vp):
        self.start_vp = start_vp
        self.node_positions = {}
        self.graph = FloydGraph()
        self.node_stop_scores = {}
        self.node_step_ids = {}

    def update_graph(self, ob):
        self.node_positions[ob['viewpoint']] = ob['position']
        p = np.asarray(ob['position'], np.float64)
        for cc in ob['candidate']:
            self.node_positions[cc['viewpointId']] = cc['position']
            q = np.asarray(cc['position'], np.float64)
            d = q - p
            dist = np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)          # calc_position_distance, :7-13
            self.graph.add_edge(ob['viewpoint'], cc['viewpointId'], dist)
        self.graph.update(ob['viewpoint'])

    def get_pos_fts(self, cur_vp, gmap_vpids, cur_heading, cur_elevation, angle_feat_size=4):
        """[n, angle_feat_size + 3]: sin / cos of the relative heading and elevation, line distance, map distance, map path length
        (graph_utils.py:127-149); None entries ([stop] / [MEM]) give the angle features of (0, 0) and zero distances."""
        n = len(gmap_vpids)
        first = 0
        while first < n and gmap_vpids[first] is None:
            first += 1
        vps = gmap_vpids[first:]
        if None in vps:             # (None entries between real nodes: not what the builders make, kept general)
            real = [i for i, vp in enumerate(gmap_vpids) if vp is not None]
            vps = [gmap_vpids[i] for i in real]
        else:
            real = slice(first, n)
        ang = np.zeros((n, 2), np.float64)
        dist = np.zeros((n, 3), np.float64)
        if vps:
            graph = self.graph
            pos = np.array([self.node_positions[vp] for vp in vps], np.float64)
            h, e, d = rel_pos(self.node_positions[cur_vp], pos)
            ang[real, 0], ang[real, 1] = h - cur_heading, e - cur_elevation
            dist[real, 0] = d / MAX_DIST
            dist[real, 1] = graph.dist_rows(cur_vp, vps) / MAX_DIST
            dist[real, 2] = np.array([graph.path_len(cur_vp, vp) for vp in vps], np.float64) / MAX_STEP
        ang = ang.astype(np.float32)
        out = np.empty((n, angle_feat_size + 3), np.float32)
        out[:, :angle_feat_size] = get_angle_fts(ang[:, 0], ang[:, 1], angle_feat_size)
        out[:, angle_feat_size:] = dist          # (float64 -> float32 on assignment, as .astype did)
        return out

    def pair_dists(self, gmap_vpids, first=2):
        """symmetric [G, G] float32 of map distances between the real nodes gmap_vpids[first:] (M/r2r/agent.py:191-195)."""
        G = len(gmap_vpids)
        out = np.zeros((G, G), np.float32)
        if G > first:
            ix = np.array([self.graph._ix(vp) for vp in gmap_vpids[first:]], dtype=np.int64)
            sub = self.graph.D[np.ix_(ix, ix)].astype(np.float32)
            np.fill_diagonal(sub, 0)
            out[first:, first:] = sub
        return out


# ------------------------------------------------------------------------------------------------ node embeddings (device)
class NodeEmbedStore:
    """`node_embeds` of B GraphMaps (graph_utils.py:98,113-125) as index bookkeeping over a pool of device rows.

    The panorama encoder's outputs of every step are appended to the pool ([B*W_t] view rows, then [B] fused rows); a node is either
    ("set", row): rewritten by its own visit, or ("acc", [rows]): the running sum of the candidate views that saw it, read back as
    the mean.  `gather` turns the current state into the CSR index of goat_gather_segmean_* over the concatenated pool; its backward
    sends each map token's gradient to the rows it averaged (inverse index: one writer per pool row, no atomics)."""

    def __init__(self, B):
        self.B = B
        self.state = [dict() for _ in range(B)]
        self.pool, self.rows = [], 0
        self._view_base = self._fused_base = self._W = None

    def advance(self, B, W):
        """row bookkeeping of one step without tensors (host-side planning: TeacherEpisode.plan)."""
        self._view_base, self._W = self.rows, W
        self.rows += B * W
        self._fused_base = self.rows
        self.rows += B

    def begin_step(self, pano_embeds, fused):
        """register this step's panorama tokens [B, W, H] and fused / averaged panorama vectors [B, H]."""
        B, W, H = pano_embeds.shape
        self.advance(B, W)
        self.pool.append(pano_embeds.reshape(B * W, H))
        self.pool.append(fused.to(pano_embeds.dtype))

    def rewrite(self, b, vp):
        """update_node_embed(vp, avg_pano_embeds[b], rewrite=True)"""
        self.state[b][vp] = ('set', self._fused_base + b)

    def accumulate(self, b, vp, j):
        """update_node_embed(vp, pano_embeds[b, j])"""
        row = self._view_base + b * self._W + j
        cur = self.state[b].get(vp)
        if cur is None:
            self.state[b][vp] = ('acc', [row])
        elif cur[0] == 'set':                       # [embed, 1] += embed: a rewritten node that is accumulated onto again
            self.state[b][vp] = ('acc', [cur[1], row])
        else:
            cur[1].append(row)

    def csr(self, gmap_vpids, G, mem_rows=None):
        """-> (idx, start, scale) int32 / int32 / float32 numpy for output token (b, g) = segment b * G + g.  Slot 0 ([stop]) is
        empty (zeros); slot 1 ([MEM]) reads pool row mem_rows[b] if given; slots >= 2 the node's rows."""
        idx, start, scale = [], [0], []
        for b in range(self.B):
            vps, state = gmap_vpids[b], self.state[b]
            n = min(max(len(vps), 2), G)
            for g in range(n):
                rows, sc = (), 1.0
                if g == 1 and mem_rows is not None:
                    rows = (mem_rows[b],)
                elif g >= 2 and g < len(vps) and vps[g] is not None:
                    kind, r = state[vps[g]]
                    if kind == 'set':
                        rows = (r,)
                    else:
                        rows, sc = r, 1.0 / len(r)
                idx.extend(rows)
                scale.append(sc)
                start.append(len(idx))
            if G > n:                           # the padding slots of the bucket: empty segments
                scale.extend([1.0] * (G - n))
                start.extend([len(idx)] * (G - n))
        if not idx:
            idx = [-1]
        return np.asarray(idx, np.int32), np.asarray(start, np.int32), np.asarray(scale, np.float32)

    def gather(self, gmap_vpids, G, last_embeds=None):
        """gmap_img_embeds [B, G, H] (M/r2r/agent.py:180-185): zeros, the previous step's [MEM] state, then the node embeddings."""
        from . import graphmap, hipops      # (lazy: CPU tests import this module)
        pool = list(self.pool)
        mem_rows = None
        if last_embeds is not None:
            mem_rows = [self.rows + b for b in range(self.B)]
            pool.append(last_embeds.to(pool[0].dtype))
        src = torch.cat(pool, 0)
        idx, start, scale = self.csr(gmap_vpids, G, mem_rows)
        inv = graphmap.inverse_index(idx, start, scale, src.shape[0])
        dev = src.device
        out = hipops.gather_segmean(src, torch.from_numpy(idx).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(scale).to(dev),
                                    self.B * G, tuple(t.to(dev) for t in inv))
        return out.view(self.B, G, src.shape[1])


# ------------------------------------------------------------------------------------------------ the navigator
class ScanGraph:
    """One building: viewpoint ids, positions [N, 3] float64, undirected adjacency (M/utils/data.py:80-105 `load_nav_graphs`)."""

    def __init__(self, name, vpids, positions, edges):
        self.name, self.vpids = name, list(vpids)
        self.index = {v: i for i, v in enumerate(self.vpids)}
        self.pos = np.asarray(positions, np.float64).reshape(len(self.vpids), 3)
        self.adj = [[] for _ in self.vpids]
        for a, b in edges:
            ia, ib = self.index[a], self.index[b]
            if ib not in self.adj[ia]:
                self.adj[ia].append(ib)
                self.adj[ib].append(ia)
        self._cands = {}
        self._sp = None

    @staticmethod
    def from_connectivity(connectivity_dir, scan):
        """Matterport3D `<scan>_connectivity.json` (list of {image_id, pose[16], included, unobstructed[]})."""
        with open(os.path.join(connectivity_dir, '%s_connectivity.json' % scan)) as f:
            data = json.load(f)
        vpids, pos, edges = [], [], []
        for i, item in enumerate(data):
            if not item['included']:
                continue
            for j, conn in enumerate(item['unobstructed']):
                if conn and data[j]['included']:
                    if item['image_id'] not in vpids:
                        vpids.append(item['image_id'])
                        pos.append([item['pose'][3], item['pose'][7], item['pose'][11]])
                    edges.append((item['image_id'], data[j]['image_id']))
        keep = set(vpids)
        return ScanGraph(scan, vpids, pos, [(a, b) for a, b in edges if a in keep and b in keep])

    @staticmethod
    def synthetic(name='scan0', n=40, seed=0, degree=3, extent=12.0):
        """random planar-ish scan: points in a box, each joined to its `degree` nearest neighbours (connected by construction:
        node i > 0 is also joined to its nearest predecessor)."""
        rs = np.random.RandomState(seed)
        pos = np.concatenate([rs.uniform(-extent, extent, (n, 2)), rs.uniform(-1.5, 1.5, (n, 1))], 1)
        vpids = ['%s_vp%03d' % (name, i) for i in range(n)]
        d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(d, np.inf)
        edges = set()
        for i in range(n):
            for j in np.argsort(d[i])[:degree]:
                edges.add((min(i, int(j)), max(i, int(j))))
            if i > 0:
                j = int(np.argmin(d[i, :i]))
                edges.add((j, i))
        return ScanGraph(name, vpids, pos, [(vpids[a], vpids[b]) for a, b in sorted(edges)])

    # all-pairs shortest distances / predecessor matrix (networkx all_pairs_dijkstra in M/r2r/env.py:183-189)
    def shortest(self):
        if self._sp is None:
            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import dijkstra
            n = len(self.vpids)
            rows, cols, w = [], [], []
            for i in range(n):
                for j in self.adj[i]:
                    rows.append(i)
                    cols.append(j)
                    w.append(float(np.sqrt(((self.pos[i] - self.pos[j]) ** 2).sum())))
            dist, pred = dijkstra(csr_matrix((w, (rows, cols)), shape=(n, n)), directed=False, return_predecessors=True)
            self._sp = (dist, pred)
        return self._sp

    def shortest_path(self, a, b):
        dist, pred = self.shortest()
        i, j = self.index[a], self.index[b]
        out = [j]
        while out[-1] != i:
            out.append(int(pred[i, out[-1]]))
        return [self.vpids[k] for k in reversed(out)]

    def candidates(self, vp):
        """make_candidate (M/r2r/env.py:241-333) for viewpoint `vp`, base-view independent part: one entry per neighbour with its
        absolute heading / elevation ('normalized_*'), the view index that sees it closest to its centre ('pointId') and its
        position, in the order the 36-view sweep first meets them."""
        got = self._cands.get(vp)
        if got is not None:
            return got
        i = self.index[vp]
        nb = self.adj[i]
        out = []
        if nb:
            h, e, _ = rel_pos(self.pos[i], self.pos[nb])
            first = []
            for n_i, (hh, ee) in enumerate(zip(h, e)):
                best, best_d, first_ix, first_d = 0, float('inf'), None, None
                for ix in range(36):
                    vh, ve = view_angles(ix)
                    rh = (hh - vh + math.pi) % (2 * math.pi) - math.pi
                    re = ee - ve
                    dd = math.sqrt(rh * rh + re * re)
                    if dd < best_d:
                        best, best_d = ix, dd
                    if first_ix is None and abs(rh) < HFOV / 2 and abs(re) < VFOV / 2:
                        first_ix, first_d = ix, dd
                if first_ix is None:
                    first_ix, first_d = best, best_d
                first.append((first_ix, first_d, n_i))
                out.append({'viewpointId': self.vpids[nb[n_i]], 'pointId': best, 'normalized_heading': float(hh),
                            'normalized_elevation': float(ee), 'position': tuple(float(x) for x in self.pos[nb[n_i]]), 'scanId': self.name,
                            'idx': n_i + 1})
            out = [out[k] for _, _, k in sorted(first)]
        self._cands[vp] = out
        return out


class ObjectStore:
    """The object half of a REVERIE / SOON observation (M/reverie/data_utils.py:46-99 `ObjectFeatureDB`; M/reverie/env.py:451-479): per
    (scan, viewpoint) up to `max_objects` detected objects with an image feature, a viewing direction (heading, elevation), a bounding
    box size (w, h in pixels of the 640 x 480 frame), an object id and a category number (`obj_name` < 45).  The features of ALL objects
    live in one [sum O, D] table that is moved to the device once (`to`); observations carry ROW numbers, and `gather` assembles a
    batch's `reverie_obj_img_fts` with the kernel that gathers the view features (FeatureStore.gather) — the 768-wide rows are never
    touched on the host.  `attributes` is `get_object_feature`: angle features relative to the agent's heading / elevation, box
    features (h / 480, w / 640, their product)."""

    def __init__(self, entries, D, dtype=torch.bfloat16, max_objects=None):
        """entries: {'<scan>_<vp>': dict(fts float32 [O, >= D], directions [O, 2], sizes [O, 2] (w, h), obj_ids [O], names int [O])}"""
        self.start, self.count, self.attrs = {}, {}, {}
        blocks, n = [], 0
        for k, e in entries.items():
            o = len(e['obj_ids']) if max_objects is None else min(len(e['obj_ids']), max_objects)
            self.start[k], self.count[k] = n, o
            self.attrs[k] = {'directions': np.asarray(e['directions'], np.float64).reshape(-1, 2)[:o], 'sizes': np.asarray(e['sizes'], np.float64).reshape(-1, 2)[:o],
                             'obj_ids': list(e['obj_ids'])[:o], 'names': np.asarray(e['names'], np.int64)[:o]}
            blocks.append(np.asarray(e['fts'], np.float32).reshape(-1, np.asarray(e['fts']).shape[-1] if len(e['obj_ids']) else D)[:o, :D])
            n += o
        tab = np.concatenate(blocks, 0) if n else np.zeros((0, D), np.float32)
        from .features import FeatureStore
        self._fs = FeatureStore.__new__(FeatureStore)               # (row gather only: the table is [sum O, D], one row per object)
        self._fs.keys, self._fs.index, self._fs.views = [], {}, 1
        self._fs.table = torch.from_numpy(np.ascontiguousarray(tab)).to(dtype)
        self._fs.dev = None
        self.D = D

    @classmethod
    def from_hdf5(cls, path, D, category_of=None, max_objects=None, dtype=torch.bfloat16):
        """The reference's object feature file (M/reverie/data_utils.py:46-78, P/data/dataset.py:838-861): one dataset '<scan>_<viewpoint>'
        [O, >= D] per viewpoint with attributes `directions` [O, 2], `sizes` [O, 2], `obj_ids` [O], `names` [O] (and `bboxes`, unused
        here).  category_of: name string -> category number (the reference's `preprocess_name` over its category-mapping files, which
        are dataset files and not part of this path); None: the names must already be numbers.  Read through h5py or, without it,
        libhdf5 (h5lite)."""
        from . import h5lite
        entries = {}
        with h5lite.open_file(path, 'r') as f:
            for key in f.keys():
                ds = f[key]
                attrs = dict(ds.attrs.items())
                names = list(np.asarray(attrs.get('names', [])).reshape(-1))
                names = [category_of(n.decode() if isinstance(n, bytes) else str(n)) for n in names] if category_of is not None else [int(n) for n in names]
                ids = [i.decode() if isinstance(i, bytes) else (i if isinstance(i, str) else (int(i) if float(i).is_integer() else i))
                       for i in np.asarray(attrs.get('obj_ids', [])).reshape(-1)]
                entries[key] = {'fts': np.asarray(ds[...], np.float32), 'directions': attrs.get('directions', np.zeros((0, 2))),
                                'sizes': attrs.get('sizes', np.zeros((0, 2))), 'obj_ids': ids, 'names': names}
        return cls(entries, D, dtype, max_objects)

    @classmethod
    def synthetic(cls, scans, D=768, max_objects=20, seed=0, dtype=torch.bfloat16, p_empty=0.2):
        """random objects on every viewpoint of the given ScanGraphs (object ids unique per scan; ~p_empty of the viewpoints see none)."""
        rs = np.random.RandomState(seed)
        entries = {}
        for scan in scans:
            next_id = 0
            for vp in scan.vpids:
                o = 0 if rs.uniform() < p_empty else int(rs.randint(1, max_objects + 1))
                entries['%s_%s' % (scan.name, vp)] = {
                    'fts': rs.standard_normal((o, D)).astype(np.float32), 'directions': np.stack([rs.uniform(0, 2 * np.pi, o), rs.uniform(-0.5, 0.5, o)], 1),
                    'sizes': np.stack([rs.uniform(20, 640, o), rs.uniform(20, 480, o)], 1), 'obj_ids': list(range(next_id, next_id + o)),
                    'names': rs.randint(0, 45, o)}
                next_id += o
        return cls(entries, D, dtype)

    def to(self, device):
        self._fs.to(device)
        return self

    def meta(self):
        """a copy WITHOUT the feature table (row numbers, directions, sizes, ids, names only): what a host-side planner needs
        (PlanWorker ships it to its worker process; `attributes` works, `gather` / `table` do not)."""
        m = ObjectStore.__new__(ObjectStore)
        m.start, m.count, m.attrs, m.D, m._fs = self.start, self.count, self.attrs, self.D, None
        return m

    @property
    def table(self):
        return self._fs.table

    def attributes(self, scan, vp, base_heading, base_elevation, angle_feat_size=4):
        """-> (rows int64 [O], obj_ang_fts [O, angle_feat_size], obj_box_fts [O, 3], obj_ids, obj_names) — get_object_feature (:80-99)."""
        k = '%s_%s' % (scan, vp)
        o, a = self.count.get(k, 0), self.attrs.get(k)
        ang = np.zeros((o, angle_feat_size), np.float32)
        box = np.zeros((o, 3), np.float32)
        if o:
            for j in range(o):
                ang[j] = angle_feature(a['directions'][j, 0] - base_heading, a['directions'][j, 1] - base_elevation, angle_feat_size)
                w, h = a['sizes'][j]
                box[j, :2] = [h / 480, w / 640]
                box[j, 2] = box[j, 0] * box[j, 1]
        rows = np.arange(self.start.get(k, 0), self.start.get(k, 0) + o, dtype=np.int64)
        return rows, ang, box, (a['obj_ids'] if o else []), (a['names'] if o else np.zeros(0, np.int64))

    def gather(self, obj_rows, out_dtype=None):
        """obj_rows int64 [B, O] (-1 = padding) on the table's device -> [B, O, D]"""
        return self._fs.gather(obj_rows, out_dtype)

    def host_rows(self, obj_rows):
        return self._fs.host_rows(obj_rows)


class GraphSim:
    """The batch of simulators of EnvBatch + R2RNavBatch._get_obs (M/r2r/env.py:26-96,335-377) on ScanGraphs.

    episodes: list of dicts {instr_id, scan (ScanGraph), path [vpids], heading, instr_encoding}.  `features`: an object with
    `row(scan_name, vpid) -> int` (features.FeatureStore): observations carry feature ROW numbers, not feature arrays."""

    def __init__(self, features=None, angle_feat_size=4, objects=None, seed=0, obj_fallback=True):
        self.features = features
        self.obj_rng = np.random.RandomState(seed)      # draws the stand-in target object of episodes without one (see _gt_obj_id)
        self.obj_fallback = obj_fallback                # False: such episodes keep gt_obj_id None (fixtures generated without the random draw)
        self.objects = objects              # ObjectStore: REVERIE / SOON observations (M/reverie/env.py:451-486); episodes then carry
        self.angle_feat_size = angle_feat_size      # 'obj_id' (the target object, may be None) and 'end_vps' (viewpoints that see it)
        self.view_angle_fts = view_angle_feature_table(angle_feat_size)
        self.batch, self.state = [], []

    def _gt_obj_id(self, ep, obj_ids):
        """target object of an observation (M/reverie/env.py:481-484): the episode's `objId`; an episode WITHOUT one (the augmented
        data) gets a random object of the current viewpoint — np.random.choice(obj_ids) there, this simulator's seeded generator here —
        so that such episodes contribute to the object-grounding loss as in the reference; None only when the viewpoint has no objects."""
        if ep.get('obj_id') is not None or len(obj_ids) == 0 or not self.obj_fallback:
            return ep.get('obj_id')
        return obj_ids[int(self.obj_rng.randint(len(obj_ids)))]

    @staticmethod
    def _snap(heading, elevation):
        """discretised viewing angles: heading / elevation snapped to the 30-degree grid, view index 0..35"""
        hs = int(round(heading / math.radians(30))) % 12
        es = min(2, max(0, int(round(elevation / math.radians(30))) + 1))
        return es * 12 + hs

    def reset(self, episodes):
        self.batch = list(episodes)
        self.state = [(ep['path'][0], self._snap(ep['heading'], 0.0)) for ep in self.batch]
        return self.observe()

    def step(self, moves):
        """moves[i] = (viewpoint, view index) or None (stay): M/r2r/agent.py:349-378 teleports with newEpisode."""
        for i, mv in enumerate(moves):
            if mv is not None:
                self.state[i] = mv
        return self.observe()

    def observe(self):
        obs = []
        for ep, (vp, view) in zip(self.batch, self.state):
            scan = ep['scan']
            bh, be = view_angles(view)
            cands = []
            for c in scan.candidates(vp):
                c = dict(c)
                c['heading'] = c['normalized_heading'] - bh
                c['elevation'] = c['normalized_elevation'] - be
                c['angle_feat'] = angle_feature(c['heading'], c['elevation'], self.angle_feat_size)
                cands.append(c)
            dist, _ = scan.shortest()
            obs.append({'instr_id': ep['instr_id'], 'scan': scan.name, 'scan_graph': scan, 'viewpoint': vp, 'viewIndex': view,
                        'position': tuple(float(x) for x in scan.pos[scan.index[vp]]), 'heading': bh, 'elevation': be,
                        'feature_row': self.features.row(scan.name, vp) if self.features is not None else -1,
                        'view_angle_fts': self.view_angle_fts[view], 'candidate': cands,
                        'instr_encoding': ep['instr_encoding'], 'gt_path': ep['path'],
                        'distance': float(dist[scan.index[vp], scan.index[ep['path'][-1]]])})
            if self.objects is not None:
                # (the simulator reports the continuous heading; on this navigator it is the snapped view's, as for the candidates)
                rows, ang, box, ids, names = self.objects.attributes(scan.name, vp, bh, be, self.angle_feat_size)
                ob = obs[-1]
                ob.update({'obj_rows': rows, 'obj_ang_fts': ang, 'obj_box_fts': box, 'obj_ids': ids, 'obj_name': names,
                           'gt_end_vps': ep.get('end_vps', []), 'gt_obj_id': self._gt_obj_id(ep, ids)})
                if ep.get('end_vps'):           # several goal viewpoints on REVERIE: distance to the nearest (env.py:493-503)
                    ob['distance'] = float(min(dist[scan.index[vp], scan.index[e]] for e in ep['end_vps']))
        return obs
