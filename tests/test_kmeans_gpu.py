"""goat_kmeans_{assign,csr,centres,pick}, DeviceKMeans and KMeansPicker on the GPU.  Every comparison is against float64 numpy computed
here from the same float32 inputs (bf16-rounded inputs in the bf16 cases); the one exception is the committed scikit-learn fit
(tests/golden/kmeans_sklearn.npz, see make_golden_kmeans.py).

Inputs.  "Gaussian": RandomState(seed).standard_normal rows with K distinct rows as centres.  "Blobs": 4 * N(0,1) blob centres plus
N(0,1) noise, one row of each blob as the initial centre.

Bounds (none of them measured on the code under test):
  - labels: equal to the float64 arg-min on every row whose float64 relative margin (d2 - d1) / d2 is >= 1e-4; on the other rows (at
    most 1 % of N) the chosen centre lies within 1e-4 relative of the best;
  - mind2: within 1e-5 * (||x||² + ||c||²) of float64 (float32 unit 6e-8, sums of up to 768 terms: about 100x head-room);
  - centres: |C - mean64| <= n_k * 2^-24 * max|X|, the worst case of ANY float32 summation order of n_k terms bounded by max|X|, divided
    by n_k, plus the rounding of the division; one missing or doubled row moves a centre by about |x| / n_k, far outside.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
ASSIGN_SHAPES = [(1037, 768, 24), (2051, 768, 256), (515, 40, 7), (300, 768, 2), (64, 8, 1), (1, 768, 24)]
ASSIGN_CASES = [(s, 'f32') for s in ASSIGN_SHAPES] + [((1037, 768, 24), 'bf16'), ((515, 40, 7), 'bf16')]


def hipops():
    from vln_goat_amd import hipops as h
    return h


def dist64(X64, C64):
    return (X64 * X64).sum(1)[:, None] - 2.0 * (X64 @ C64.T) + (C64 * C64).sum(1)[None, :]


def margins(d):
    """-> (arg-min, best distance, relative margin to the second best); one centre: the margin is infinite."""
    best = d.argmin(1)
    if d.shape[1] == 1:
        return best, d[:, 0], np.full(len(d), np.inf)
    part = np.partition(d, 1, axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        m = (part[:, 1] - part[:, 0]) / part[:, 1]
    return best, part[:, 0], np.where(part[:, 1] > 0, m, 0.0)


def check_labels(labels, d, what=''):
    """the margin rule of the module docstring"""
    N = len(d)
    best, d1, m = margins(d)
    assert labels.min() >= 0 and labels.max() < d.shape[1], what
    clear = m >= 1e-4
    print('%s: %d of %d rows under the 1e-4 margin; %d labels differ from the float64 arg-min' % (what, (~clear).sum(), N, (labels != best).sum()))
    assert (~clear).sum() <= 0.01 * N, what
    assert np.array_equal(labels[clear], best[clear]), what
    chosen = d[np.arange(N), labels]
    assert np.all(chosen[~clear] <= d1[~clear] + 1e-4 * np.abs(d1[~clear])), what


@functools.lru_cache(maxsize=None)
def gaussian(N, D, K, dtype, seed=11):
    """-> X (device, float32 or bfloat16), C (device float32), X64, C64 (numpy, the values the device sees), all read-only."""
    rs = np.random.RandomState(seed + N + D + K)
    pool = rs.standard_normal((max(N, K), D)).astype(np.float32)
    C = pool[rs.choice(len(pool), K, replace=False)].copy()
    X = torch.from_numpy(pool[:N].copy())
    if dtype == 'bf16':
        X = X.bfloat16()
    X64 = X.float().double().numpy()
    return X.to(DEV), torch.from_numpy(C).to(DEV), X64, C.astype(np.float64)


@functools.lru_cache(maxsize=None)
def assigned(N, D, K, dtype):
    """One assign step from labels = -1 on the Gaussian case, and a second one on its own output: shared by the tests below."""
    X, C, X64, C64 = gaussian(N, D, K, dtype)
    changed = torch.zeros(1, dtype=torch.int32, device=DEV)
    labels, mind2 = hipops().kmeans_assign(X, C, None, None, changed)
    first = int(changed.item())
    l1, m1 = labels.cpu().numpy().copy(), mind2.cpu().numpy().copy()
    hipops().kmeans_assign(X, C, labels, mind2, changed)
    second = int(changed.item())
    return l1, m1, first, second, labels.cpu().numpy(), dist64(X64, C64)


# ------------------------------------------------------------------------------------------------ assign
@pytest.mark.parametrize('shape,dtype', ASSIGN_CASES, ids=['%dx%dx%d-%s' % (s + (d,)) for s, d in ASSIGN_CASES])
def test_assign_labels_and_distances(shape, dtype):
    N, D, K = shape
    labels, mind2, first, second, labels2, d = assigned(N, D, K, dtype)
    check_labels(labels, d, 'assign %s %s' % (shape, dtype))
    _, _, X64, C64 = gaussian(N, D, K, dtype)
    chosen = d[np.arange(N), labels]
    bound = 1e-5 * ((X64 * X64).sum(1) + (C64 * C64).sum(1)[labels])
    err = np.abs(mind2.astype(np.float64) - np.maximum(chosen, 0.0))
    print('mind2: largest error / bound = %.3g' % float((err / bound).max()))
    assert np.all(err <= bound)
    assert first == N                                   # every row moved away from -1
    assert second == N and np.array_equal(labels2, labels)      # the same inputs again: nothing moves, the counter is only added to


def test_assign_tie_goes_to_the_lowest_index_and_nan_counts_as_inf():
    X, C, X64, C64 = gaussian(1037, 768, 24, 'f32')
    C2 = C.clone()
    C2[5] = C2[2]
    labels, _ = hipops().kmeans_assign(X, C2)
    labels = labels.cpu().numpy()
    assert not (labels == 5).any() and (labels == 2).any()
    C64b = C64.copy()
    C64b[5] = 1e3                                       # float64 reference without the duplicate: 5 is nobody's nearest
    check_labels(labels, dist64(X64, C64b), 'tie')
    C3 = C.clone()
    C3[0] = float('nan')                                # a NaN centre scores +inf: never chosen while a finite one exists
    labels3, _ = hipops().kmeans_assign(X, C3)
    labels3 = labels3.cpu().numpy()
    assert not (labels3 == 0).any()
    C64c = C64.copy()
    C64c[0] = 1e3
    check_labels(labels3, dist64(X64, C64c), 'nan')


def test_assign_strided_rows():
    """ld_x > D: the rows of a wider table"""
    N, D, K = 515, 40, 7
    rs = np.random.RandomState(5)
    wide = torch.from_numpy(rs.standard_normal((N, 64)).astype(np.float32)).to(DEV)
    X = wide[:, :D]
    C = X[:K].contiguous()
    labels, _ = hipops().kmeans_assign(X, C)
    X64 = X.double().cpu().numpy()
    check_labels(labels.cpu().numpy(), dist64(X64, X64[:K]), 'strided')


# ------------------------------------------------------------------------------------------------ CSR and centres
def csr_checks(labels, start, order, K):
    N = len(labels)
    valid = (labels >= 0) & (labels < K)
    counts = np.bincount(labels[valid], minlength=K)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(order[:start[K]], np.argsort(np.where(valid, labels, K), kind='stable')[:start[K]])     # grouped, ascending inside
    if valid.all():
        assert np.array_equal(np.sort(order), np.arange(N))


@pytest.mark.parametrize('shape', [(1037, 768, 24), (2051, 768, 256), (515, 40, 7)], ids=lambda s: '%dx%dx%d' % s)
def test_csr_and_centres(shape):
    N, D, K = shape
    X, C, X64, _ = gaussian(N, D, K, 'f32')
    labels = assigned(N, D, K, 'f32')[0]
    lab = torch.from_numpy(labels).to(DEV)
    start, order = hipops().kmeans_csr(lab, K)
    s, o = start.cpu().numpy(), order.cpu().numpy()
    csr_checks(labels, s, o, K)
    sentinel = 12345.0
    out = torch.full((K, D), sentinel, device=DEV)
    hipops().kmeans_centres(X, order, start, out)
    again = torch.full((K, D), sentinel, device=DEV)
    hipops().kmeans_centres(X, order, start, again)
    assert torch.equal(out, again)                      # a fixed reduction order: the same bits
    got = out.cpu().numpy().astype(np.float64)
    xmax = np.abs(X64).max()
    worst = 0.0
    for k in range(K):
        n = s[k + 1] - s[k]
        if n == 0:
            assert np.all(got[k] == sentinel)
            continue
        err = np.abs(got[k] - X64[labels == k].mean(0)).max()
        worst = max(worst, err / (n * 2.0 ** -24 * xmax))
        assert err <= n * 2.0 ** -24 * xmax, (k, n, err)
    print('centres %s: largest error / bound = %.3g' % (shape, worst))


def test_centres_bf16_rows():
    N, D, K = 515, 40, 7
    X, C, X64, _ = gaussian(N, D, K, 'bf16')
    labels = assigned(N, D, K, 'bf16')[0]
    start, order = hipops().kmeans_csr(torch.from_numpy(labels).to(DEV), K)
    out = hipops().kmeans_centres(X, order, start, torch.zeros(K, D, device=DEV)).cpu().numpy().astype(np.float64)
    for k in range(K):
        n = int((labels == k).sum())
        if n:
            assert np.abs(out[k] - X64[labels == k].mean(0)).max() <= n * 2.0 ** -24 * np.abs(X64).max()


def test_one_cluster_holds_every_row():
    N, D, K = 4099, 72, 3                                # 72 columns: three column slabs, the last one partial
    rs = np.random.RandomState(2)
    Xh = rs.standard_normal((N, D)).astype(np.float32)
    X = torch.from_numpy(Xh).to(DEV)
    lab = torch.ones(N, dtype=torch.int32, device=DEV)
    start, order = hipops().kmeans_csr(lab, K)
    assert start.tolist() == [0, 0, N, N]
    assert torch.equal(order, torch.arange(N, dtype=torch.int32, device=DEV))
    out = torch.full((K, D), -7.0, device=DEV)
    hipops().kmeans_centres(X, order, start, out)
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(got[0] == -7.0) and np.all(got[2] == -7.0)
    assert np.abs(got[1] - Xh.astype(np.float64).mean(0)).max() <= N * 2.0 ** -24 * np.abs(Xh).max()
    again = torch.full((K, D), -7.0, device=DEV)
    hipops().kmeans_centres(X, order, start, again)
    assert torch.equal(out, again)


def test_two_of_256_clusters_in_use_and_labels_out_of_range():
    N, D, K = 777, 40, 256
    rs = np.random.RandomState(8)
    Xh = rs.standard_normal((N, D)).astype(np.float32)
    labels = np.where(rs.rand(N) < 0.4, 3, 200).astype(np.int32)
    X = torch.from_numpy(Xh).to(DEV)
    start, order = hipops().kmeans_csr(torch.from_numpy(labels).to(DEV), K)
    csr_checks(labels, start.cpu().numpy(), order.cpu().numpy(), K)
    out = torch.full((K, D), 99.0, device=DEV)
    hipops().kmeans_centres(X, order, start, out)
    got = out.cpu().numpy().astype(np.float64)
    used = np.zeros(K, bool)
    used[[3, 200]] = True
    assert np.all(got[~used] == 99.0)
    for k in (3, 200):
        n = int((labels == k).sum())
        assert np.abs(got[k] - Xh[labels == k].astype(np.float64).mean(0)).max() <= n * 2.0 ** -24 * np.abs(Xh).max()
    # labels outside [0, K) are skipped: start[K] < N
    bad = labels.copy()
    bad[::10] = -1
    bad[5::10] = 256
    start, order = hipops().kmeans_csr(torch.from_numpy(bad).to(DEV), K)
    s = start.cpu().numpy()
    assert s[K] == int(((bad >= 0) & (bad < K)).sum()) < N
    csr_checks(bad, s, order.cpu().numpy(), K)


# ------------------------------------------------------------------------------------------------ pick
def _pick_case(N=168, D=40, K=24, dtype=torch.float32, skip=None):
    rs = np.random.RandomState(21)
    X = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32)).to(DEV).to(dtype)
    labels = np.arange(N) % K                            # 7 members per cluster
    if skip is not None:
        labels[labels == skip] = (skip + 1) % K
    rs.shuffle(labels)
    lab = torch.from_numpy(labels.astype(np.int32)).to(DEV)
    start, order = hipops().kmeans_csr(lab, K)
    return X, labels, start, order


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_pick_members_copies_and_reproducibility(dtype):
    K, B = 24, 3
    X, labels, start, order = _pick_case(dtype=dtype)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((B, K, X.shape[1]), 5.0, device=DEV, dtype=dtype)
    picked = hipops().kmeans_pick(X, order, start, out, seed=77, offset=9, rng_dev=ctr).cpu().numpy()
    assert np.array_equal(labels[picked], np.arange(K))                 # every pick is a member of its cluster
    for b in range(B):
        assert torch.equal(out[b], X[torch.from_numpy(picked).long().to(DEV)])
    out2 = torch.zeros_like(out)
    again = hipops().kmeans_pick(X, order, start, out2, seed=77, offset=9, rng_dev=ctr).cpu().numpy()
    assert np.array_equal(again, picked) and torch.equal(out, out2)     # the same (seed, offset, counter): the same picks
    no_ctr = hipops().kmeans_pick(X, order, start, out2, seed=77, offset=9).cpu().numpy()
    assert np.array_equal(no_ctr, picked)                               # a counter of 0 and no counter are the same draw
    ctr += 1
    bumped = hipops().kmeans_pick(X, order, start, out2, seed=77, offset=9, rng_dev=ctr).cpu().numpy()
    assert np.array_equal(labels[bumped], np.arange(K))
    assert not np.array_equal(bumped, picked)           # 24 clusters of 7: the chance of no change is 7^-24
    by_seed = hipops().kmeans_pick(X, order, start, out2, seed=78, offset=9).cpu().numpy()
    assert not np.array_equal(by_seed, picked)


def test_pick_is_uniform_over_the_members():
    N, D, draws = 8, 8, 800
    X = torch.arange(N, dtype=torch.float32, device=DEV).repeat_interleave(D).view(N, D).contiguous()
    start, order = hipops().kmeans_csr(torch.zeros(N, dtype=torch.int32, device=DEV), 1)
    picked = torch.empty(draws, 1, dtype=torch.int32, device=DEV)
    out = torch.empty(1, 1, D, device=DEV)
    for i in range(draws):
        hipops().kmeans_pick(X, order, start, out, picked[i], seed=3, offset=i)
    counts = np.bincount(picked.cpu().numpy().ravel(), minlength=N)
    sigma = np.sqrt(draws * (1 / 8) * (7 / 8))
    print('pick counts over 800 draws:', counts.tolist(), ' 5 sigma = %.1f' % (5 * sigma))
    assert counts.sum() == draws and len(counts) == N
    assert np.all(np.abs(counts - draws / N) <= 5 * sigma)


def test_pick_empty_cluster():
    K, B = 24, 2
    X, labels, start, order = _pick_case(skip=4)
    out = torch.full((B, K, X.shape[1]), 5.0, device=DEV)
    picked = hipops().kmeans_pick(X, order, start, out, seed=1).cpu().numpy()
    assert picked[4] == -1 and torch.all(out[:, 4] == 0)
    rest = np.arange(K) != 4
    assert np.array_equal(labels[picked[rest]], np.arange(K)[rest])


# ------------------------------------------------------------------------------------------------ blobs, fits
def blobs(N, D, K, seed, spread=4.0):
    """-> X float32 [N, D], blob ids [N] (every blob has rows), the first row of every blob in blob order."""
    rs = np.random.RandomState(seed)
    centres = spread * rs.standard_normal((K, D))
    ids = np.arange(N) % K
    rs.shuffle(ids)
    X = (centres[ids] + rs.standard_normal((N, D))).astype(np.float32)
    first = np.array([np.flatnonzero(ids == k)[0] for k in range(K)])
    return X, ids, first


def means64(X64, labels, K):
    return np.stack([X64[labels == k].mean(0) for k in range(K)])


def centre_bound(labels, K, X64):
    return (np.bincount(labels, minlength=K) * 2.0 ** -24 * np.abs(X64).max())[:, None]


def test_fit_blobs():
    from vln_goat_amd.frontdoor import DeviceKMeans
    N, D, K = 1037, 768, 24
    Xh, ids, first = blobs(N, D, K, seed=31)
    X = torch.from_numpy(Xh).to(DEV)
    km = DeviceKMeans(K, tol=0, init=X[torch.from_numpy(first).to(DEV)]).fit(X)
    labels = km.labels_.cpu().numpy()
    assert np.array_equal(labels, ids)
    assert km.n_iter_ == 2
    X64 = Xh.astype(np.float64)
    inertia = float(((X64 - means64(X64, ids, K)[ids]) ** 2).sum())
    print('inertia: %.9g, float64 %.9g' % (km.inertia_, inertia))
    assert abs(km.inertia_ - inertia) <= 1e-5 * inertia
    csr_checks(labels, km.start_.cpu().numpy(), km.order_.cpu().numpy(), K)
    assert np.all(np.abs(km.cluster_centers_.cpu().numpy() - means64(X64, ids, K)) <= centre_bound(ids, K, X64))


def test_fit_gaussian_reaches_a_fixed_point():
    from vln_goat_amd.frontdoor import DeviceKMeans
    N, D, K = 1037, 768, 24
    X, C, X64, _ = gaussian(N, D, K, 'f32')
    km = DeviceKMeans(K, tol=0, init=C).fit(X)
    labels = km.labels_.cpu().numpy()
    cen = km.cluster_centers_.cpu().numpy().astype(np.float64)
    print('gaussian fit: %d assign steps, inertia %.6g' % (km.n_iter_, km.inertia_))
    assert 2 <= km.n_iter_ <= 300
    check_labels(labels, dist64(X64, cen), 'fixed point')              # one float64 assign step on the centres gives the labels back
    assert np.bincount(labels, minlength=K).min() > 0
    assert np.all(np.abs(cen - means64(X64, labels, K)) <= centre_bound(labels, K, X64))


def refill_reference(X64, C, max_steps=50):
    """The refill rule restated in float64 numpy: a cluster left empty by an assign step takes the row with the largest distance to its
    own centre (several: descending distance, ties to the lowest index, empty clusters ascending) for THIS centre update; the row
    leaves its old cluster's mean and keeps its label.  -> labels, centres, assign steps, the smallest relative margin seen (between
    distinct centres, and between the rows competing for a refill)."""
    K = len(C)
    C = C.copy()
    labels, steps, margin = None, 0, np.inf
    while steps < max_steps:
        d = dist64(X64, C)
        new = d.argmin(1)                                # numpy's arg-min takes the first of equal values: the lowest index
        steps += 1
        _, keep = np.unique(C, axis=0, return_index=True)
        margin = min(margin, float(margins(d[:, np.sort(keep)])[2].min()))
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        mind2 = d[np.arange(len(d)), labels]
        empty = np.flatnonzero(np.bincount(labels, minlength=K) == 0)
        moved = labels.copy()
        if len(empty):
            far = np.argsort(-mind2, kind='stable')[:len(empty) + 1]
            margin = min(margin, float(np.min(-np.diff(mind2[far]) / mind2[far[:-1]])))
            moved[far[:len(empty)]] = empty
        for k in range(K):
            if (moved == k).any():
                C[k] = X64[moved == k].mean(0)
    return labels, C, steps, margin


def test_fit_refills_an_empty_cluster():
    from vln_goat_amd.frontdoor import DeviceKMeans
    N, D, K = 300, 40, 3
    Xh, ids, first = blobs(N, D, K, seed=13)
    init = Xh[first].copy()
    init[1] = init[0]                                    # centre 1 loses every tie against centre 0: empty after the first assign
    X64 = Xh.astype(np.float64)
    labels, cen, steps, margin = refill_reference(X64, init.astype(np.float64))
    assert margin >= 1e-3, margin                        # a check of the INPUT: no float32 step can legitimately differ
    assert steps >= 3 and np.bincount(labels, minlength=K).min() > 0
    X = torch.from_numpy(Xh).to(DEV)
    km = DeviceKMeans(K, tol=0, init=torch.from_numpy(init)).fit(X)
    got = km.labels_.cpu().numpy()
    assert np.array_equal(got, labels)
    assert km.n_iter_ == steps
    assert np.all(np.abs(km.cluster_centers_.cpu().numpy() - cen) <= centre_bound(labels, K, X64))


def test_kmeanspp_init():
    from vln_goat_amd.frontdoor import DeviceKMeans
    X, _, _, _ = gaussian(515, 40, 7, 'f32')
    runs = []
    for seed in (0, 0, 1):
        km = DeviceKMeans(7, max_iter=0, seed=seed).fit(X)          # max_iter = 0: the centres are the initial ones
        rows = km.init_rows_.cpu().numpy()
        assert len(np.unique(rows)) == 7
        assert torch.equal(km.cluster_centers_, X[km.init_rows_.long()])
        assert km.n_iter_ == 1
        runs.append(rows)
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], runs[2])
    # two blobs 40 apart: the second centre is drawn in proportion to the squared distance to the first, so it falls in the first's own
    # blob with probability about 16 / (16 + 1616) = 1 % (D = 8).  Twenty seeds, at most two such draws: P(more) < 1.1e-3.
    rs = np.random.RandomState(4)
    ids = np.arange(64) % 2
    Xb = rs.standard_normal((64, 8))
    Xb[:, 0] += 40.0 * ids
    Xb = torch.from_numpy(Xb.astype(np.float32)).to(DEV)
    same = 0
    for seed in range(20):
        rows = DeviceKMeans(2, max_iter=0, seed=seed).fit(Xb).init_rows_.cpu().numpy()
        same += int(ids[rows[0]] == ids[rows[1]])
    assert same <= 2, same


def test_fit_raises_on_a_cluster_that_stays_empty():
    from vln_goat_amd.frontdoor import DeviceKMeans
    X = torch.ones(16, 8, device=DEV)                    # identical rows: nothing can fill a second cluster
    with pytest.raises(ValueError, match='empty'):
        DeviceKMeans(2, max_iter=3, init=torch.ones(2, 8)).fit(X)


def test_fit_matches_the_sklearn_golden(golden_dir):
    from vln_goat_amd.frontdoor import DeviceKMeans
    spec = importlib.util.spec_from_file_location('make_golden_kmeans', os.path.join(golden_dir, 'make_golden_kmeans.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(os.path.join(golden_dir, 'kmeans_sklearn.npz'))
    Xh, init_rows = gen.make_case(int(z['seed']))
    assert np.array_equal(init_rows, z['init_rows'])
    X = torch.from_numpy(Xh).to(DEV)
    km = DeviceKMeans(gen.K, tol=0, init=X[torch.from_numpy(z['init_rows']).to(DEV)]).fit(X)
    labels = km.labels_.cpu().numpy()
    assert np.array_equal(labels, z['labels'])
    assert km.n_iter_ == int(z['steps'])
    X64 = Xh.astype(np.float64)
    assert np.all(np.abs(km.cluster_centers_.cpu().numpy() - z['centres']) <= centre_bound(labels, gen.K, X64))


# ------------------------------------------------------------------------------------------------ the picker
@functools.lru_cache(maxsize=None)
def picker_case():
    from vln_goat_amd.frontdoor import KMeansPicker
    tables = {}
    for i, k in enumerate(('txt_feats', 'vp_feats', 'gmap_feats')):
        Xh, _, _ = blobs(96, 16, 4, seed=40 + i)
        tables[k] = torch.from_numpy(Xh).to(DEV)
    return KMeansPicker(tables, None, 4, DEV, seed=5), tables


def test_picker_dictionaries_are_members():
    picker, tables = picker_case()
    d = picker.random_pick_front_features()
    assert sorted(d) == ['gmap_feats', 'txt_feats', 'vp_feats']
    for k, x in tables.items():
        km = picker.kmeans_model_dict[k]
        rows = picker.picked_[k].long()
        assert tuple(d[k].shape) == (4, 16) and d[k].dtype == torch.float32
        assert torch.equal(d[k], x[rows])
        assert torch.equal(km.labels_[rows].cpu(), torch.arange(4, dtype=torch.int32))


def test_picker_extras_are_rewritten_in_place_under_a_captured_graph():
    picker, tables = picker_case()
    ex = picker.extras(3)
    assert sorted(ex) == ['language', 'navigation']
    assert sorted(ex['navigation']) == ['front_gmap_feats', 'front_txt_feats', 'front_vp_feats'] and list(ex['language']) == ['front_txt_feats']
    buf = ex['navigation']['front_vp_feats']
    assert tuple(buf.shape) == (3, 4, 16)
    ptrs = {m: {k: t.data_ptr() for k, t in v.items()} for m, v in ex.items()}
    before_rows = picker.picked_['vp_feats'].clone()
    assert torch.equal(buf, tables['vp_feats'][before_rows.long()].expand(3, 4, 16))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf.to(torch.bfloat16)                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # one stream, one cast: no parallel branches
        cast = buf.to(torch.bfloat16)
    graph.replay()
    assert torch.equal(cast, buf.to(torch.bfloat16))
    counter = int(picker.counter_.item())
    d = picker.random_pick_front_features()
    assert int(picker.counter_.item()) == counter + 1
    # 4 clusters of 24 rows: the chance that none of the four vp picks moved is 24^-4 = 3e-6
    assert not torch.equal(picker.picked_['vp_feats'], before_rows)
    ex2 = picker.extras(3)
    assert {m: {k: t.data_ptr() for k, t in v.items()} for m, v in ex2.items()} == ptrs
    assert torch.equal(buf, d['vp_feats'].expand(3, 4, 16))
    assert torch.equal(ex2['language']['front_txt_feats'], d['txt_feats'].expand(3, 4, 16))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cast, d['vp_feats'].to(torch.bfloat16).expand(3, 4, 16))
    # bf16 buffers follow the same picks
    exb = picker.extras(2, torch.bfloat16)
    d = picker.random_pick_front_features()
    assert torch.equal(exb['navigation']['front_gmap_feats'], d['gmap_feats'].to(torch.bfloat16).expand(2, 4, 16))
    assert torch.equal(buf, d['vp_feats'].expand(3, 4, 16))


def test_picker_save_and_reload(tmp_path):
    from vln_goat_amd.frontdoor import KMeansPicker, read_tim_tsv
    picker, tables = picker_case()
    picker.save(str(tmp_path / 'km'))
    again = KMeansPicker(tables, str(tmp_path / 'km'), 4, DEV, seed=5)
    for k in tables:
        assert torch.equal(again.kmeans_model_dict[k].labels_, picker.kmeans_model_dict[k].labels_)
        assert torch.equal(again.kmeans_model_dict[k].order_, picker.kmeans_model_dict[k].order_)
    d = again.random_pick_front_features()
    tsv = str(tmp_path / 'frontdoor_update_features.tsv')
    again.save_features(tsv)
    back = read_tim_tsv(tsv)
    for a, k in zip(back, ('txt_feats', 'vp_feats', 'gmap_feats')):
        assert a.shape == (4, 16) and np.array_equal(a, d[k].cpu().numpy())
