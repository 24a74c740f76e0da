"""Regenerates tests/golden/kmeans_sklearn.npz: a Lloyd fit by scikit-learn that DeviceKMeans must reproduce label for label.

    python tests/golden/make_golden_kmeans.py          (CPU; written with scikit-learn 1.7.2)

Recipe: three blobs (centres 0.5 * N(0,1), rows = centre + N(0,1)), N = 151, D = 768, K = 6, six distinct random rows as initial
centres, KMeans(n_clusters=6, init=C0, n_init=1, algorithm='lloyd', tol=0) on the float64 copy of the float32 rows.  With three
blobs under six centres the fit has real work to do (rows change sides for several iterations), unlike well separated blobs.

The script walks the seeds until a case (a) takes at least 4 assign steps, (b) keeps a float64 relative margin (d2 - d1) / d2 between
best and second-best centre of at least 5e-4 on every row at EVERY step (so a float32 assign step cannot legitimately differ), and
(c) never empties a cluster; (a)-(c) are asserted on a float64 Lloyd loop written out below, and scikit-learn must agree with that
loop on labels, centres and step count.  Stored: the seed, the initial row indices, the labels, the float64 centres, the step count —
the test regenerates X from the seed with make_case().
"""
import os

import numpy as np

N, D, K, N_BLOBS, SCALE = 151, 768, 6, 3, 0.5
MIN_STEPS, MIN_MARGIN = 4, 5e-4


def make_case(seed):
    """-> X float32 [N, D], init_rows int64 [K] (numpy RandomState: bit-stable across machines)."""
    rs = np.random.RandomState(seed)
    centres = SCALE * rs.standard_normal((N_BLOBS, D))
    blob = rs.randint(0, N_BLOBS, N)
    X = (centres[blob] + rs.standard_normal((N, D))).astype(np.float32)
    init_rows = rs.choice(N, K, replace=False)
    return X, init_rows


def lloyd64(X, C):
    """float64 Lloyd, tol = 0: -> labels, centres, assign steps, smallest relative margin over all steps, ever-empty flag."""
    X = X.astype(np.float64)
    C = C.astype(np.float64).copy()
    labels, steps, margin = None, 0, np.inf
    while True:
        d = ((X * X).sum(1)[:, None] - 2.0 * X @ C.T + (C * C).sum(1)[None, :])
        part = np.partition(d, 1, axis=1)
        margin = min(margin, float(((part[:, 1] - part[:, 0]) / part[:, 1]).min()))
        new = d.argmin(1)
        steps += 1
        if labels is not None and np.array_equal(new, labels):
            return labels, C, steps, margin, False
        labels = new
        counts = np.bincount(labels, minlength=K)
        if (counts == 0).any():
            return labels, C, steps, margin, True
        C = np.stack([X[labels == k].mean(0) for k in range(K)])


def main():
    from sklearn.cluster import KMeans
    for seed in range(1000):
        X, init_rows = make_case(seed)
        labels, C, steps, margin, emptied = lloyd64(X, X[init_rows])
        if steps >= MIN_STEPS and margin >= MIN_MARGIN and not emptied:
            break
    else:
        raise SystemExit('no seed below 1000 meets the conditions')
    assert steps >= MIN_STEPS and margin >= MIN_MARGIN and not emptied
    X64 = X.astype(np.float64)
    km = KMeans(n_clusters=K, init=X64[init_rows], n_init=1, algorithm='lloyd', tol=0).fit(X64)
    assert np.array_equal(km.labels_, labels), 'scikit-learn and the float64 loop disagree on labels'
    assert km.n_iter_ == steps, (km.n_iter_, steps)
    assert np.abs(km.cluster_centers_ - C).max() <= 1e-12 * np.abs(X64).max() * N
    assert np.bincount(km.labels_, minlength=K).min() > 0
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'kmeans_sklearn.npz')
    np.savez_compressed(out, seed=np.int64(seed), init_rows=init_rows.astype(np.int64), labels=km.labels_.astype(np.int32),
                        centres=km.cluster_centers_.astype(np.float64), steps=np.int64(steps), margin=np.float64(margin))
    print('seed %d: %d assign steps, smallest margin %.3g, cluster sizes %s -> %s (%d bytes)'
          % (seed, steps, margin, np.bincount(km.labels_, minlength=K).tolist(), out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
