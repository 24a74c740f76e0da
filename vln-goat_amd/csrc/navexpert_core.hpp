// The nDTW expert of a policy-driven walk, one episode at a time (csrc/navstate.hip launches it behind the step kernel): the DAgger
// label of `_teacher_action` under expert_policy = 'ndtw' (M/r2r/agent.py:330-346), which the RxR scripts set.  Per selectable
// unvisited map node the reference runs `cal_dtw` (M/r2r/eval_utils.py:6-26) over (walked path + shortest path to the node) x
// (ground-truth path) and keeps the first node whose -nDTW is strictly smallest.  Here all candidates of an episode share the DTW
// row of the path walked so far: it is kept between steps and folded forward by the hops the step kernel logged; per candidate what is
// left are the rows of shortest_path(cur, candidate)[1:], one thread per candidate.
//
// Bit-exactness.  A row is filled serially, cell j = dist[node][ref[j - 1]] + min(up, left, diag), float64, one IEEE addition per
// cell in cal_dtw's order; the (min, +) recurrence along a row is NOT turned into a scan across lanes, which would reassociate the
// additions.  The parallelism is over the candidates.
// The kernel compares DTW, not -nDTW = -exp(-DTW / (3 R)): exp is monotone, so the two orders agree except where rounding maps two
// different DTWs to one double, and the device's exp is not numpy's — comparing nDTW here would be the LESS faithful choice.  (The
// host restatement, nav_inputs.teacher_action, keeps np.exp.)
//
// Written like navstate_core.hpp: `tid` of `nt` threads and a `sync` callable, no HIP type; compiles as plain C++ with (0, 1, no-op).
#pragma once
#include "navstate_core.hpp"

namespace navstate {

struct Expert {
  const int32_t* ref;      // [B, max_ref + 1]: the length of the ground-truth path, then its viewpoint numbers
  double* xd;              // B blocks of expert_doubles(cap, max_ref)
  int max_ref;
};

// float64 words of an episode: the DTW row behind the last folded node of the walked path [max_ref + 1], then one working row per
// map node, interleaved (cell j of node c at (max_ref + 1) + j * cap + c: the threads of a wave touch neighbouring words)
NAV_HD inline int expert_doubles(int cap, int max_ref) { return (cap + 1) * (max_ref + 1); }

// one row of cal_dtw in place: row = dtw_matrix[i - 1] becomes dtw_matrix[i] for the prediction node whose distances are `drow`
NAV_HD inline void dtw_row(double* row, int stride, const double* drow, const int32_t* ref, int off, int R) {
#pragma clang fp contract(off)
  double diag = row[0], left = INFINITY;
  row[0] = INFINITY;
  for (int j = 1; j <= R; ++j) {
    const double up = row[(int64_t)j * stride];
    double m = up;                       // min(dtw[i-1][j], dtw[i][j-1], dtw[i-1][j-1])
    if (left < m) m = left;
    if (diag < m) m = diag;
    const double c = drow[ref[j] - off] + m;
    row[(int64_t)j * stride] = c;
    diag = up;
    left = c;
  }
}

// The label of step a.t for episode b, written over what build_episode put into the step's `target`.  Collective.
// row_s / ref_s: room for max_ref + 1 doubles / ints all threads share (LDS), or both null: the fold then works on global memory.
template <class Sync>
NAV_HD inline void ndtw_label(const Args& a, const Expert& x, int b, int tid, int nt, Sync sync, double* row_s = nullptr,
                              int32_t* ref_s = nullptr) {
  Ep e(a, b);
  const Layout& L = e.L;
  const int32_t* S = e.S;
  const int cap = a.cap, stride = x.max_ref + 1;
  const int cur = e.H[H_CUR], goal = e.H[H_GOAL], nslots = e.H[H_NSLOT];
  int64_t* target = step_ptr<int64_t>(a, TB_TARGET) + b;
  if (e.H[H_ENDED] || cur == goal) {          // (the walked path is folded when a label next needs it)
    if (tid == 0) *target = e.H[H_ENDED] ? a.ignoreid : 0;
    return;
  }
  const int32_t* ref_g = x.ref + (int64_t)b * stride;
  double* row_g = x.xd + (int64_t)b * expert_doubles(cap, x.max_ref);
  double* work = row_g + stride;
  int R = ref_g[0];
  if (R < 1 || R > x.max_ref) {              // begin() refuses such a path: keep the step kernel's label
    if (tid == 0) e.fail(ST_PATH, a.t);
    return;
  }
  const int s = e.H[H_SCAN];
  const int off = scan_ptr<int32_t>(a, SC_SCAN_OFF)[s], ns = scan_ptr<int32_t>(a, SC_SCAN_N)[s];
  const double* dist = scan_ptr<double>(a, SC_DIST) + scan_ptr<int64_t>(a, SC_DIST_OFF)[s];
  const int32_t* prow = scan_ptr<int32_t>(a, SC_PRED) + scan_ptr<int64_t>(a, SC_DIST_OFF)[s] + (int64_t)(cur - off) * ns;
  const int32_t* ref = ref_s ? ref_s : ref_g;
  double* row = row_s ? row_s : row_g;
  const int folded = e.H[H_FOLD];
  if (row_s) {
    for (int j = tid; j <= R; j += nt) {
      ref_s[j] = ref_g[j];
      row_s[j] = folded ? row_g[j] : (j == 0 ? 0.0 : INFINITY);
    }
    sync();
  }
  // ---- fold: the start viewpoint and every hop logged since the last label, one row each, serially
  if (tid == 0) {
    if (!row_s && !folded)
      for (int j = 0; j <= R; ++j) row[j] = j == 0 ? 0.0 : INFINITY;
    const int want = 1 + e.hs[a.t];
    int f = folded;
    for (; f < want; ++f) {
      const int node = f == 0 ? e.H[H_START] : e.hops[f - 1];
      dtw_row(row, 1, dist + (int64_t)(node - off) * ns, ref, off, R);
    }
    e.H[H_FOLD] = f;
  }
  sync();
  if (row_s)
    for (int j = tid; j <= R; j += nt) row_g[j] = row_s[j];
  // ---- one thread per selectable unvisited node: the rows of shortest_path(cur, node)[1:] behind the shared prefix
  const int c0 = cur - off;
  for (int g = 2 + tid; g < nslots; g += nt) {
    const int node = S[L.o_ord + g - 2];
    if (S[L.o_vis + node]) continue;
    double* w = work + node;
    const int k = S[L.o_vp + node] - off;
    int len = 0;                              // hops of the predecessor chain from the node back to cur
    for (int v = k; v != c0; ++len) {
      v = (v >= 0 && v < ns && len < ns) ? prow[v] : -1;
      if (v < 0 || v >= ns) {
        len = -1;
        break;
      }
    }
    w[(int64_t)R * cap] = INFINITY;
    if (len < 0) {
      e.fail(ST_PATH, a.t);
      w[0] = -1.0;                            // no candidate
      continue;
    }
    for (int j = 0; j <= R; ++j) w[(int64_t)j * cap] = row[j];
    for (int i = len - 1; i >= 0; --i) {      // the chain comes out reversed: re-walk it to the i-th node from its end
      int v = k;
      for (int q = 0; q < i; ++q) v = prow[v];
      dtw_row(w, cap, dist + (int64_t)v * ns, ref, off, R);
    }
  }
  sync();
  // ---- strict <, the first minimum in slot order wins
  if (tid == 0) {
    int64_t best_g = a.ignoreid;
    double best = INFINITY;
    for (int g = 2; g < nslots; ++g) {
      const int node = S[L.o_ord + g - 2];
      if (S[L.o_vis + node]) continue;
      const double* w = work + node;
      if (w[0] < 0.0) continue;
      const double d = w[(int64_t)R * cap];
      if (best_g == a.ignoreid || d < best) {      // (-nDTW < inf holds for every DTW)
        best = d;
        best_g = g;
      }
    }
    *target = best_g;
  }
}

}  // namespace navstate
