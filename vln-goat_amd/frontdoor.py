"""The front-door (FACL) dictionary pipeline on the device: pooled features of the training set -> k-means per modality -> one
random member per cluster, redrawn during training.

Reference: M/r2r/agent.py:1008-1049 (extract_cfp_features: the loop and the four-field TSV), M/utils/data.py:403-480 (KMeansPicker:
sklearn KMeans per modality, np.random.choice per cluster, save_features), M/r2r/main_nav.py:182-188,316-324 (the re-pick every
update_iter iterations and after a new best validation score), M/r2r/agent.py:497-512 (the copy per sample).

What differs from the reference:
  - features, labels, centres and dictionaries are device tensors ([N, H] tables, [K, H] dictionaries), not lists of numpy rows;
  - the fit is Lloyd's algorithm on the goat_kmeans_* kernels (csrc/kmeans.hip) with a seeded k-means++ start of its own: it follows
    sklearn's stopping and empty-cluster rules but does not reproduce sklearn's random draws;
  - `kmeans_file` / save() are a directory of `<modality>.npz` files (labels, centres).  sklearn / joblib pickles are NOT read;
  - a cluster that ends up empty raises ValueError (the reference would silently return a shorter dictionary);
  - a re-pick rewrites persistent buffers in place and bumps a device counter, so an episode graph captured over extras() sees the
    new dictionaries on its next replay: no re-capture, no host copy.
"""
import base64
import csv
import os

import numpy as np
import torch

from . import hipops

TIM_TSV_FIELDNAMES = ['path_id', 'txt_feats', 'vp_feats', 'gmap_feats']
FEAT_KEYS = tuple(TIM_TSV_FIELDNAMES[1:])
_OUTPUT_KEYS = {'txt_feats': 'txt_outputs', 'vp_feats': 'vp_outputs', 'gmap_feats': 'gmap_outputs'}


# ----------------------------------------------------------------------------- the reference's TSV (base64 of float32 rows, no header)
def read_tim_tsv(path, return_dict=False):
    """M/utils/data.py:430-449: -> (txt, vp, gmap) float32 arrays [N, H], or {'txt_feats': [row, ...], ...} with return_dict (the shape
    validation hands to the agent as z_front_dict).  See read_tim_tsv_ids for the first column."""
    feats = {k: [] for k in FEAT_KEYS}
    with open(path, 'rt') as f:
        for item in csv.DictReader(f, delimiter='\t', fieldnames=TIM_TSV_FIELDNAMES):
            for k in FEAT_KEYS:
                feats[k].append(np.frombuffer(base64.b64decode(item[k]), dtype=np.float32))
    if return_dict:
        return feats
    return tuple(np.array(feats[k]) for k in FEAT_KEYS)


def read_tim_tsv_ids(path):
    """The path_id column of a TIM TSV, as strings."""
    with open(path, 'rt') as f:
        return [item['path_id'] for item in csv.DictReader(f, delimiter='\t', fieldnames=TIM_TSV_FIELDNAMES)]


def _rows(a):
    if torch.is_tensor(a):
        a = a.detach().float().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def write_tim_tsv(path, path_ids, txt, vp, gmap):
    """Write the file M/r2r/agent.py:1037-1049 writes (r2r_cfp_features.tsv): one line per row, `path_id <tab> base64(float32 row)` x 3.
    txt / vp / gmap: [N, H] tensors or arrays.  path_ids: a sequence of N ids, or ONE id for every line — write_tim_tsv(path, 0, ...)
    with the [n_clusters, H] dictionaries is the reference's save_features (frontdoor_update_features.tsv, --frontdoor_dict_file)."""
    cols = [_rows(txt), _rows(vp), _rows(gmap)]
    n = len(cols[0])
    if any(c.ndim != 2 or len(c) != n for c in cols):
        raise ValueError('write_tim_tsv: txt, vp and gmap must be [N, H] with one N, got %s' % [c.shape for c in cols])
    ids = [path_ids] * n if isinstance(path_ids, (int, str)) else list(path_ids)
    if len(ids) != n:
        raise ValueError('write_tim_tsv: %d path ids for %d rows' % (len(ids), n))
    with open(path, 'wt') as f:
        writer = csv.DictWriter(f, delimiter='\t', fieldnames=TIM_TSV_FIELDNAMES)
        for i in range(n):
            rec = {'path_id': ids[i]}
            for k, c in zip(FEAT_KEYS, cols):
                rec[k] = str(base64.b64encode(c[i]), 'utf-8')
            writer.writerow(rec)


# ----------------------------------------------------------------------------- extraction
def extract_front_features(model, batches):
    """The loop of M/r2r/agent.py:1008-1035: model('extract_cfp_features', batch) under no_grad for every collated batch of `batches`
    (any iterable; the schema is the one nav_model.extract_cfp_features takes).  -> {'txt_feats', 'vp_feats', 'gmap_feats'}: float32
    [N, H] tables that stay on the device, rows in batch order."""
    parts = {k: [] for k in FEAT_KEYS}
    with torch.no_grad():
        for batch in batches:
            out = model('extract_cfp_features', batch)
            for k in FEAT_KEYS:
                parts[k].append(out[_OUTPUT_KEYS[k]].detach().float())
    if not parts['txt_feats']:
        raise ValueError('extract_front_features: no batches')
    return {k: torch.cat(v, 0).contiguous() for k, v in parts.items()}


# ----------------------------------------------------------------------------- k-means
class DeviceKMeans:
    """Lloyd's k-means on the device (sklearn.cluster.KMeans(algorithm='lloyd', n_init=1) in spirit).

    Per iteration: goat_kmeans_assign -> goat_kmeans_csr -> goat_kmeans_centres, and ONE host read (the count of rows whose label
    changed, the count of empty clusters, and whether the previous centre update moved less than the tolerance).  The fit stops when no
    label changed, when the squared centre shift is <= tol * mean(var(X, axis=0)) (the labels are then those of one more assign step
    on the final centres, as in sklearn), or after max_iter centre updates (likewise).  A cluster left empty by an assign step takes the
    row farthest from its own centre as its new centre (several: in descending distance, ties to the lowest row index, empty clusters
    in ascending order); that row leaves its old cluster's mean and keeps its label for the iteration.  Still empty at return:
    ValueError.  init: 'k-means++' (seeded; not sklearn's draws) or a [K, D] tensor.

    After fit(): labels_ int32 [N], cluster_centers_ float32 [K, D], inertia_ (float), n_iter_ (assign steps run), and the membership
    index start_ int32 [K+1] / order_ int32 [N] (cluster k = order_[start_[k]:start_[k+1]], ascending)."""

    def __init__(self, n_clusters, max_iter=300, tol=1e-4, init='k-means++', seed=0):
        if not 1 <= int(n_clusters) <= hipops.KMEANS_MAXK:
            raise ValueError('DeviceKMeans: n_clusters = %d, the kernels serve 1..%d' % (n_clusters, hipops.KMEANS_MAXK))
        self.n_clusters, self.max_iter, self.tol, self.init, self.seed = int(n_clusters), int(max_iter), float(tol), init, int(seed)

    def _kmeanspp(self, X):
        N, K = X.shape[0], self.n_clusters
        gen = torch.Generator(device=X.device)
        gen.manual_seed(self.seed)
        idx = torch.randint(N, (1,), generator=gen, device=X.device)
        rows = [idx]
        running = torch.full((N,), float('inf'), device=X.device)
        scratch = torch.empty(N, dtype=torch.int32, device=X.device)
        d2 = torch.empty(N, device=X.device)
        for _ in range(1, K):
            hipops.kmeans_assign(X, X[idx].float().contiguous(), scratch, d2)        # K = 1: the distance to the newest centre
            running = torch.minimum(running, d2)
            running[idx] = 0.0                                                        # (its own distance may round to a tiny positive)
            idx = torch.multinomial(running, 1, generator=gen)
            rows.append(idx)
        self.init_rows_ = torch.cat(rows)
        return X[self.init_rows_].float().contiguous()

    def fit(self, X):
        hipops._inference_only('DeviceKMeans.fit', X)
        if X.dim() != 2 or X.shape[0] < self.n_clusters:
            raise ValueError('DeviceKMeans.fit: X is [N, D] with N >= n_clusters = %d, got %s' % (self.n_clusters, tuple(X.shape)))
        X = X.contiguous()
        N, D = X.shape
        K = self.n_clusters
        if torch.is_tensor(self.init):
            if tuple(self.init.shape) != (K, D):
                raise ValueError('DeviceKMeans.fit: init is [%d, %d], got %s' % (K, D, tuple(self.init.shape)))
            C = self.init.detach().to(device=X.device, dtype=torch.float32).contiguous().clone()
        elif self.init == 'k-means++':
            C = self._kmeanspp(X)
        else:
            raise ValueError("DeviceKMeans: init is 'k-means++' or a [K, D] tensor")
        tol_abs = self.tol * float(X.float().var(dim=0, unbiased=False).mean()) if self.tol > 0 else 0.0
        labels = torch.full((N,), -1, dtype=torch.int32, device=X.device)
        mind2 = torch.empty(N, dtype=torch.float32, device=X.device)
        changed = torch.zeros(1, dtype=torch.int32, device=X.device)
        small = torch.zeros((), dtype=torch.int32, device=X.device)      # did the last centre update move <= tol_abs
        n_iter = 0
        while True:
            changed.zero_()
            hipops.kmeans_assign(X, C, labels, mind2, changed)
            n_iter += 1
            start, order = hipops.kmeans_csr(labels, K)
            empty = (start[1:] == start[:-1])
            n_changed, n_empty, is_small = torch.stack([changed[0], empty.sum().to(torch.int32), small]).tolist()
            if n_changed == 0 or is_small or n_iter > self.max_iter:
                break
            C_old = C.clone() if tol_abs > 0 else None
            if n_empty:
                # the farthest rows stand in for the empty clusters in THIS centre update only (labels keeps what the assign step gave)
                far = torch.sort(mind2, descending=True, stable=True).indices[:n_empty]
                moved = labels.clone()
                moved[far] = torch.nonzero(empty).flatten().to(torch.int32)
                m_start, m_order = hipops.kmeans_csr(moved, K)
                hipops.kmeans_centres(X, m_order, m_start, C)
            else:
                hipops.kmeans_centres(X, order, start, C)
            if C_old is not None:
                small = ((C - C_old) ** 2).sum().le(tol_abs).to(torch.int32)
        if n_empty:
            raise ValueError('DeviceKMeans.fit: %d of %d clusters are empty after %d assign steps' % (n_empty, K, n_iter))
        self.labels_, self.cluster_centers_, self.start_, self.order_, self.n_iter_ = labels, C, start, order, n_iter
        self.inertia_ = float((X.float() - C[labels.long()]).double().pow(2).sum())
        return self


# ----------------------------------------------------------------------------- the picker
class KMeansPicker:
    """M/utils/data.py:403-480 with the reference's name and argument order.  front_feat_file_or_tables: the path of a TIM TSV, or
    {'txt_feats', 'vp_feats', 'gmap_feats'} -> [N, H] tables (what extract_front_features returns).  kmeans_file: a directory written
    by save() (`<modality>.npz` with labels and centres; sklearn / joblib pickles are NOT read) — without it the three fits run here.

    random_pick_front_features() -> {'txt_feats', 'vp_feats', 'gmap_feats'}: [K, H] float32 device tensors, one uniformly drawn member
    per cluster; picked_[modality] holds the row indices (int32 [K]).  The returned tensors and everything extras() handed out are
    PERSISTENT: every pick rewrites them in place (goat_kmeans_pick) and then adds one to counter_ (int64 [1] on the device, owned by
    the picker; the draws are a function of seed + counter_)."""

    def __init__(self, front_feat_file_or_tables, kmeans_file=None, n_clusters=256, device='cuda', seed=0):
        self.TIM_TSV_FIELDNAMES = TIM_TSV_FIELDNAMES
        self.n_clusters, self.seed = int(n_clusters), int(seed)
        self.device = torch.device(device)
        src = front_feat_file_or_tables
        if isinstance(src, (str, os.PathLike)):
            src = dict(zip(FEAT_KEYS, read_tim_tsv(src)))
        self.feat_dicts = {}
        for k in FEAT_KEYS:
            t = src[k]
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)) if not torch.is_tensor(t) else t.detach()
            self.feat_dicts[k] = t.to(device=self.device, dtype=torch.float32).contiguous()
        self.kmeans_model_dict = {}
        for i, (k, x) in enumerate(self.feat_dicts.items()):
            km = DeviceKMeans(self.n_clusters, seed=self.seed + i)
            if kmeans_file is not None:
                z = np.load(os.path.join(kmeans_file, k + '.npz'))
                km.labels_ = torch.from_numpy(z['labels'].astype(np.int32)).to(self.device)
                km.cluster_centers_ = torch.from_numpy(z['centres'].astype(np.float32)).to(self.device)
                if km.labels_.numel() != x.shape[0] or tuple(km.cluster_centers_.shape) != (self.n_clusters, x.shape[1]):
                    raise ValueError('KMeansPicker: %s.npz does not fit %d rows / %d clusters' % (k, x.shape[0], self.n_clusters))
                km.start_, km.order_ = hipops.kmeans_csr(km.labels_, self.n_clusters)
                if bool((km.start_[1:] == km.start_[:-1]).any()):
                    raise ValueError('KMeansPicker: %s.npz has empty clusters' % k)
            else:
                km.fit(x)
            self.kmeans_model_dict[k] = km
        H = {k: x.shape[1] for k, x in self.feat_dicts.items()}
        self.counter_ = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.picked_ = {k: torch.empty(self.n_clusters, dtype=torch.int32, device=self.device) for k in FEAT_KEYS}
        self._dicts = {k: torch.zeros(1, self.n_clusters, H[k], device=self.device) for k in FEAT_KEYS}
        self._tables = {torch.float32: self.feat_dicts}      # dtype -> tables (goat_kmeans_pick copies rows, it does not convert)
        self._n_picks = 0
        self._extras = {}                                    # (B, dtype) -> {modality: [B, K, H]}

    def _pick_into(self, bufs, dtype):
        for i, k in enumerate(FEAT_KEYS):
            km = self.kmeans_model_dict[k]
            hipops.kmeans_pick(self._tables[dtype][k], km.order_, km.start_, bufs[k], self.picked_[k], seed=self.seed,
                               offset=i * hipops.KMEANS_MAXK, rng_dev=self.counter_)

    def random_pick_front_features(self):
        with torch.no_grad():
            self._pick_into(self._dicts, torch.float32)
            for (B, dtype), bufs in self._extras.items():    # the same (seed, offset, counter): the same rows
                self._pick_into(bufs, dtype)
            self.counter_ += 1
        self._n_picks += 1
        return {k: v[0] for k, v in self._dicts.items()}

    def extras(self, B, dtype=None):
        """The 'language' / 'navigation' front-door entries of synth.rollout_extras as [B, K, H] buffers of `dtype` (default float32)
        holding the current dictionaries.  One set of buffers per (B, dtype), handed out again on every call and rewritten in place
        by every later pick."""
        dtype = dtype or torch.float32
        key = (int(B), dtype)
        if key not in self._extras:
            if dtype not in self._tables:
                self._tables[dtype] = {k: x.to(dtype) for k, x in self.feat_dicts.items()}
            if self._n_picks == 0:
                self.random_pick_front_features()
            self._extras[key] = {k: self._dicts[k].to(dtype).repeat(key[0], 1, 1) for k in FEAT_KEYS}
        b = self._extras[key]
        return {'language': {'front_txt_feats': b['txt_feats']},
                'navigation': {'front_txt_feats': b['txt_feats'], 'front_vp_feats': b['vp_feats'], 'front_gmap_feats': b['gmap_feats']}}

    def save(self, directory):
        """Store labels and centres of the three fits as <directory>/<modality>.npz (read back through kmeans_file=directory)."""
        os.makedirs(directory, exist_ok=True)
        for k, km in self.kmeans_model_dict.items():
            np.savez(os.path.join(directory, k + '.npz'), labels=km.labels_.cpu().numpy(), centres=km.cluster_centers_.cpu().numpy())

    def save_features(self, target_file, feat_data=None):
        """M/utils/data.py:468-480: the dictionaries (default: the current pick) as a TIM TSV with path_id 0, n_clusters lines."""
        d = feat_data if feat_data is not None else {k: v[0] for k, v in self._dicts.items()}
        write_tim_tsv(target_file, 0, d['txt_feats'], d['vp_feats'], d['gmap_feats'])
