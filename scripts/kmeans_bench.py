"""Times frontdoor.DeviceKMeans.fit and one KMeansPicker.random_pick_front_features() at the size class of the R2R training split
(about 14 000 pooled rows of 768) and writes profiles/kmeans_fit.txt.

    python scripts/kmeans_bench.py [--rows 14039] [--out profiles/kmeans_fit.txt]

Per K in (24, 256): Gaussian blobs (4 * N(0,1) centres, N(0,1) noise, K blobs), K random rows as initial centres, tol = 1e-4, median of
5 timed runs after 2 warm-ups; the fit's time is wall clock around fit() + a final synchronize, so its host reads are included.  When
scikit-learn imports, sklearn.cluster.KMeans(algorithm='lloyd', n_init=1) from the same initial centres is timed on the host cores
(median of 3) for scale; the two fits stop by the same rules but are not required to take the same number of steps.
"""
import argparse
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vln_goat_amd import frontdoor, hipops  # noqa: E402


def blobs(N, D, K, seed):
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.standard_normal((K, D))
    ids = rs.randint(0, K, N)
    X = (centres[ids] + rs.standard_normal((N, D))).astype(np.float32)
    return X, rs.choice(N, K, replace=False)


def median_ms(fn, warm, runs):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def cpu_name():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=14039)
    ap.add_argument('--dim', type=int, default=768)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_fit.txt'))
    args = ap.parse_args()
    threads = int(os.environ.get('OMP_NUM_THREADS', '0')) or torch.get_num_threads()
    lines = ['k-means fit and dictionary pick (scripts/kmeans_bench.py): %d x %d float32 rows, Gaussian blobs' % (args.rows, args.dim),
             'device: %s   host: %s, %d threads' % (torch.cuda.get_device_name(0), cpu_name(), threads),
             'DeviceKMeans: tol 1e-4, init = K random rows, median of 5 after 2 warm-ups (min .. max), host reads included', '']
    try:
        from sklearn.cluster import KMeans
    except Exception as e:          # noqa: BLE001
        KMeans = None
        lines.append('scikit-learn does not import here (%s): no host figure' % type(e).__name__)
    for K in (24, 256):
        Xh, rows = blobs(args.rows, args.dim, K, seed=K)
        X = torch.from_numpy(Xh).cuda()
        init = X[torch.from_numpy(rows).cuda()].clone()
        km = frontdoor.DeviceKMeans(K, init=init)
        med, lo, hi = median_ms(lambda: km.fit(X), 2, 5)
        lines.append('K = %3d  DeviceKMeans.fit      %9.3f ms (%.3f .. %.3f)  %d assign steps, inertia %.6g, %.3f ms per step'
                     % (K, med, lo, hi, km.n_iter_, km.inertia_, med / km.n_iter_))
        labels = torch.full((args.rows,), -1, dtype=torch.int32, device='cuda')
        mind2 = torch.empty(args.rows, device='cuda')
        for name, fn in (('goat_kmeans_assign', lambda: hipops.kmeans_assign(X, km.cluster_centers_, labels, mind2)),
                         ('goat_kmeans_csr', lambda: hipops.kmeans_csr(km.labels_, K)),
                         ('goat_kmeans_centres', lambda: hipops.kmeans_centres(X, km.order_, km.start_, km.cluster_centers_.clone()))):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            lines.append('         %-22s %9.1f us per call (20 back-to-back calls between two events, allocations of the wrapper included)'
                         % (name, e0.elapsed_time(e1) * 1e3 / 20))
        picker = frontdoor.KMeansPicker({k: X for k in frontdoor.FEAT_KEYS}, None, K, 'cuda')      # (three k-means++ fits, not timed)
        picker.extras(8)
        med, lo, hi = median_ms(picker.random_pick_front_features, 2, 5)
        lines.append('K = %3d  random_pick_front_features (3 modalities, [K, H] + extras(8)) %9.3f ms (%.3f .. %.3f)' % (K, med, lo, hi))
        if KMeans is not None:
            C0 = Xh[rows]
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                sk = KMeans(n_clusters=K, init=C0, n_init=1, algorithm='lloyd', tol=1e-4).fit(Xh)
                times.append((time.perf_counter() - t0) * 1e3)
            lines.append('K = %3d  sklearn KMeans.fit    %9.3f ms (median of 3, %d threads)  n_iter_ %d, inertia %.6g'
                         % (K, statistics.median(times), threads, sk.n_iter_, sk.inertia_))
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
