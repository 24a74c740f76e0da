// goat_nav_metrics: every per-trajectory score of the validation metrics (M/r2r/env.py:452-490 `_eval_item`, M/r2r/eval_utils.py
// `cal_dtw` / `cal_cls`, and the goal-set rule of M/reverie/env.py:543-549) in ONE launch over N items.  The reference walks Python
// loops per item over dict-of-dict distance tables: O(P R) table lookups for DTW and again for CLS.
//
// ONE wave (64 threads) per item.  The item's scan selects a packed row-major [n, n] float64 table; pred / ref are node indices.
//   * DTW by anti-diagonals: cell (i, j) of the reference's (P + 1) x (R + 1) matrix lies on diagonal d = i + j and reads (i - 1, j),
//     (i, j - 1) from diagonal d - 1 and (i - 1, j - 1) from d - 2.  Three diagonals live in LDS, indexed by the reference position j;
//     lanes stride over the cells of a diagonal, one barrier per diagonal.  Every cell is cost + min(three exact values): the same
//     single add the reference performs, so the matrix — and DTW — is bit-identical to it.  The borders (0 at (0, 0), inf elsewhere in
//     row / column 0) are formed from the indices, not stored.  P is not capped; R <= max_ref sizes the LDS.
//   * path lengths, the nearest-to-goal minimum, the goal-set membership and the CLS coverage are lane-strided loops closed by a
//     butterfly over the wave (every lane ends with the same value).  Sums are float64; their order differs from numpy's pairwise sum.
//   * lane 0 writes the item's GOAT_NAV_METRICS_COLS values with plain stores.  No atomics.
// An item the kernel cannot evaluate (scan id outside [0, n_scans), P < 1, R < 1, R > max_ref) gets a row of NaN and touches no table.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int NM_MAXREF = 2047;

struct NavMetricsArgs {
  const double* dist;
  const int64_t* scan_off;
  const int32_t* scan_n;
  const int32_t* item_scan;
  const int32_t* pred;
  const int32_t* pred_start;
  const int32_t* ref;
  const int32_t* ref_start;
  const int32_t* goal;
  const int32_t* goal_start;
  int n_scans, max_ref;
  double margin;
  double* out;
};

__device__ __forceinline__ double nm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double nm_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int nm_wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// sum of table[nodes[k]][nodes[k + 1]], k < n - 1
__device__ __forceinline__ double nm_path_length(const double* D, int ns, const int32_t* nodes, int n, int lane) {
  double s = 0.0;
  for (int k = lane; k + 1 < n; k += 64) s += D[(int64_t)nodes[k] * ns + nodes[k + 1]];
  return nm_wave_sum(s);
}

__global__ __launch_bounds__(64) void nav_metrics_kernel(NavMetricsArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double nm_lds[];
  const int n = blockIdx.x, lane = threadIdx.x;
  double* out = a.out + (int64_t)n * GOAT_NAV_METRICS_COLS;
  const int s = a.item_scan[n];
  const int p0 = a.pred_start[n], P = a.pred_start[n + 1] - p0;
  const int r0 = a.ref_start[n], R = a.ref_start[n + 1] - r0;
  if (s < 0 || s >= a.n_scans || P < 1 || R < 1 || R > a.max_ref) {      // (block-uniform)
    if (lane < GOAT_NAV_METRICS_COLS) out[lane] = NAN;
    return;
  }
  const int ns = a.scan_n[s];
  const double* D = a.dist + a.scan_off[s];
  const int32_t* p = a.pred + p0;
  const int32_t* r = a.ref + r0;
  const int W = a.max_ref + 1;
  double* diag = nm_lds;                                       // [3][W]
  int32_t* rl = reinterpret_cast<int32_t*>(nm_lds + 3 * W);    // [max_ref]: the reference path
  for (int j = lane; j < R; j += 64) rl[j] = r[j];
  const int goal_node = r[R - 1], last = p[P - 1];

  // ---- errors, lengths, success (M/r2r/env.py:470-483) ----
  const double nav_error = D[(int64_t)last * ns + goal_node];
  double nearest = INFINITY;
  for (int i = lane; i < P; i += 64) nearest = fmin(nearest, D[(int64_t)p[i] * ns + goal_node]);
  const double oracle_error = nm_wave_min(nearest);
  const double traj_len = nm_path_length(D, ns, p, P, lane);
  const double gt_len = nm_path_length(D, ns, r, R, lane);
  double success, oracle_success;
  if (a.goal) {                                                // M/reverie/env.py:543-549: the goal viewpoints of the item's object
    const int g0 = a.goal_start[n], g1 = a.goal_start[n + 1];
    int hit_last = 0, hit_any = 0;
    for (int i = lane; i < P; i += 64) {
      const int v = p[i];
      for (int g = g0; g < g1; ++g) hit_any |= (a.goal[g] == v);
    }
    for (int g = g0 + lane; g < g1; g += 64) hit_last |= (a.goal[g] == last);
    success = nm_wave_or(hit_last) ? 1.0 : 0.0;
    oracle_success = nm_wave_or(hit_any) ? 1.0 : 0.0;
  } else {
    success = nav_error < a.margin ? 1.0 : 0.0;
    oracle_success = oracle_error < a.margin ? 1.0 : 0.0;
  }
  const double spl = success * gt_len / fmax(fmax(traj_len, gt_len), 0.01);

  // ---- DTW (eval_utils.cal_dtw) ----
  __syncthreads();                                             // rl is complete
  for (int d = 2; d <= P + R; ++d) {
    double* cur = diag + (d % 3) * W;
    const double* d1 = diag + ((d + 2) % 3) * W;
    const double* d2 = diag + ((d + 1) % 3) * W;
    const int jlo = d - P > 1 ? d - P : 1, jhi = d - 1 < R ? d - 1 : R;
    for (int j = jlo + lane; j <= jhi; j += 64) {
      const int i = d - j;
      const double up = i == 1 ? INFINITY : d1[j];                                   // (i - 1, j)
      const double left = j == 1 ? INFINITY : d1[j - 1];                             // (i, j - 1)
      const double dg = (i == 1 && j == 1) ? 0.0 : ((i == 1 || j == 1) ? INFINITY : d2[j - 1]);      // (i - 1, j - 1)
      const double cost = D[(int64_t)p[i - 1] * ns + rl[j - 1]];
      cur[j] = cost + fmin(fmin(up, left), dg);
    }
    __syncthreads();
  }
  const double dtw = diag[((P + R) % 3) * W + R];
  const double ndtw = exp(-dtw / (a.margin * (double)R));
  const double sdtw = success * ndtw;

  // ---- CLS (eval_utils.cal_cls) ----
  double cov = 0.0;
  for (int j = lane; j < R; j += 64) {
    const double* row = D + (int64_t)rl[j] * ns;
    double m = INFINITY;
    for (int i = 0; i < P; ++i) m = fmin(m, row[p[i]]);
    cov += exp(-m / a.margin);
  }
  const double coverage = nm_wave_sum(cov) / (double)R;
  const double expected = coverage * gt_len;
  const double score = expected / (expected + fabs(expected - traj_len));
  const double cls = coverage * score;

  if (lane == 0) {
    out[0] = nav_error;
    out[1] = oracle_error;
    out[2] = (double)(P - 1);
    out[3] = traj_len;
    out[4] = gt_len;
    out[5] = success;
    out[6] = oracle_success;
    out[7] = spl;
    out[8] = dtw;
    out[9] = ndtw;
    out[10] = sdtw;
    out[11] = cls;
  }
}

}  // namespace

extern "C" int goat_nav_metrics(void* stream, const double* dist, const int64_t* scan_off, const int32_t* scan_n, int n_scans,
                                const int32_t* item_scan, const int32_t* pred, const int32_t* pred_start, const int32_t* ref,
                                const int32_t* ref_start, const int32_t* goal, const int32_t* goal_start, int N, int max_ref, double margin,
                                double* out) {
  if (!dist || !scan_off || !scan_n || !item_scan || !pred || !pred_start || !ref || !ref_start || !out) return GOAT_E_ARG;
  if ((goal == nullptr) != (goal_start == nullptr)) return GOAT_E_ARG;
  if (N < 1 || n_scans < 1 || max_ref < 1 || max_ref > NM_MAXREF) return GOAT_E_SHAPE;
  NavMetricsArgs a = {dist, scan_off, scan_n, item_scan, pred, pred_start, ref, ref_start, goal, goal_start, n_scans, max_ref, margin, out};
  const size_t lds = (size_t)3 * (max_ref + 1) * sizeof(double) + (size_t)max_ref * sizeof(int32_t);
  hipLaunchKernelGGL(nav_metrics_kernel, dim3(N), dim3(64), lds, ST(stream), a);
  GOAT_LAUNCH_CHECK();
  return 0;
}
