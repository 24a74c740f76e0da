// goat_nav_reset / goat_nav_step: the navigator of a policy-driven walk on the device, so that a sampled or argmax walk is one
// loop of launches without a host table, a host decision or a read-back per step.  A step for index t does what the host planner's
// EpisodePlanner.advance() of step t - 1 followed by build_step() of step t do (vln-goat_amd/episodes.py:245-357), which restate
//   * the map:        GraphMap.update_graph / FloydGraph.add_edge, update, path        M/models/graph_utils.py:43-144
//   * the move:       stop / no-node-left / last-step rules, make_equiv_action        M/r2r/agent.py:349-378,601-672
//   * the action:     Categorical(probs).sample() as an inverse CDF, or the argmax    M/r2r/agent.py:629-660
//   * the tables:     _panorama_feature_variable, _nav_gmap_variable, _nav_vp_variable, _teacher_action   M/r2r/agent.py:82-347
//   * the logit fusion matrix                                                          M/models/vilmodel_GOAT.py:790-806
// The text of all of it is csrc/navstate_core.hpp.
//
// This is latency-bound work on a few hundred values per episode, not bandwidth: ONE workgroup of 256 threads per episode.  The
// order-dependent parts (node insertion, the action, path expansion, map order, the DAgger label) run on thread 0; the Floyd
// relaxation over [n, n] and the [G], [G, G], [G, W + 2] and [W] tables are spread over the threads between barriers.  The state of an
// episode stays in HBM / L2 between steps; the float64 distance matrix and the predecessor matrix are read there (at cap = 126 nodes
// the two are 190 KB, more than a workgroup's LDS), the node lists and the header (a few KB) are copied into LDS for the step: the
// serial parts are chains of dependent loads over them, each a fraction of a trip to L2 when it comes from LDS.  Every value
// that must equal the host's bit for bit is one IEEE operation with contraction off.  A second launch of ONE workgroup forms the
// batch-wide compact CSRs (prefix sums over the episodes, fixed order, no atomics).
// goat_nav_ndtw is a third, optional launch behind the two: the DAgger label of the nDTW expert (csrc/navexpert_core.hpp) over the
// step kernel's shortest-path label, for walks whose TeacherEpisode has expert_policy = 'ndtw'.
// Errors (a map wider than the bucket, a panorama wider than W, an action that is no selectable node) become a sticky status word
// per episode; the kernel clamps and goes on.
#include "common.hpp"

#define NAV_HD __host__ __device__
#include "navstate_core.hpp"
#include "navexpert_core.hpp"

namespace {

using namespace navstate;

struct DevSync {
  __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(256) void nav_reset_kernel(Args a, const int32_t* ep) {
  reset_episode(a, ep, blockIdx.x, threadIdx.x, blockDim.x, DevSync());
}

// the node lists and the header of the episode are staged in LDS: the serial parts walk them in chains of dependent loads
__global__ __launch_bounds__(256) void nav_step_kernel(Args a) {
  extern __shared__ int32_t nav_lds[];
  step_episode(a, blockIdx.x, threadIdx.x, blockDim.x, DevSync(), nav_lds);
}

__global__ __launch_bounds__(256) void nav_tail_kernel(Args a) {
  __shared__ int32_t part[256];
  nav_tail(a, part, threadIdx.x, blockDim.x, DevSync());
}

// goat_nav_ndtw (the comment of csrc/navexpert_core.hpp says what it restates): one workgroup per episode behind the step kernel.  The
// ground-truth path and the shared DTW row are staged in LDS for the serial fold; the candidates' rows stay in HBM / L2.
__global__ __launch_bounds__(256) void nav_ndtw_kernel(Args a, Expert x) {
  __shared__ double row_s[GOAT_NAV_MAX_REF + 1];
  __shared__ int32_t ref_s[GOAT_NAV_MAX_REF + 1];
  ndtw_label(a, x, blockIdx.x, threadIdx.x, blockDim.x, DevSync(), row_s, ref_s);
}

// objects: a REVERIE / SOON walk, whose O is a bucket of 1..GOAT_NAV_MAX_O object slots; an R2R walk has O = 0
int nav_sizes_bad(int B, int T, int W, int O, int cap, bool objects) {
  return B < 1 || B > GOAT_NAV_MAX_B || T < 1 || T > GOAT_NAV_MAX_T || W < 1 || W > GOAT_NAV_MAX_W || cap < 1 || cap > GOAT_NAV_MAX_CAP ||
         (objects ? O < 1 || O > GOAT_NAV_MAX_O : O != 0);
}

// the walk's own fields first; a reset leaves everything behind `cap` zero, goat_nav_ndtw everything behind `step_tab`
Args nav_args(const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, int B, int T, int W, int O, int cap, int t = 0,
              int64_t ignoreid = 0, const int64_t* step_tab = nullptr, int32_t* ws = nullptr, const void* act = nullptr,
              const double* u = nullptr, int mode = 0, int Gp = 0, int G = 0, int A = 0, const int64_t* obj_tab = nullptr,
              const int64_t* ostep_tab = nullptr, const int32_t* goal = nullptr, int max_end = 0) {
  return {scan_tab, step_tab, si, sd, log, ws, act, u, mode, t, B, T, Gp, G, W, A, cap, ignoreid, obj_tab, ostep_tab, goal, O, max_end};
}

// a missing pointer (`rest`: those of the entry point beside the state) is GOAT_E_ARG, ahead of GOAT_E_SHAPE for the sizes
int nav_check(const Args& a, bool objects, bool rest) {
  if (!a.scan_tab || !a.si || !a.sd || !a.log || !rest) return GOAT_E_ARG;
  return nav_sizes_bad(a.B, a.T, a.W, a.O, a.cap, objects) ? GOAT_E_SHAPE : 0;
}

int nav_reset(void* stream, const Args& a, const int32_t* ep, bool objects) {
  if (const int bad = nav_check(a, objects, ep)) return bad;
  hipLaunchKernelGGL(nav_reset_kernel, dim3(a.B), dim3(256), 0, ST(stream), a, ep);
  GOAT_LAUNCH_CHECK();
  return 0;
}

// the step kernel and, where step t has tables (t < T), the batch-wide tail behind it
int nav_step(void* stream, const Args& a, bool objects) {
  const int t = a.t, T = a.T;
  if (const int bad = nav_check(a, objects, a.ws && (!objects || (a.obj_tab && a.goal)))) return bad;
  if ((objects && (a.max_end < 1 || a.max_end > GOAT_NAV_MAX_END)) || t < 0 || t > T) return GOAT_E_SHAPE;
  if (a.mode != MODE_SAMPLE && a.mode != MODE_ARGMAX && a.mode != MODE_FORCED) return GOAT_E_ARG;
  if (t < T && (!a.step_tab || (objects && !a.ostep_tab))) return GOAT_E_ARG;
  if (t > 0 && (!a.act || (a.mode == MODE_SAMPLE && !a.u))) return GOAT_E_ARG;
  if (t < T && (a.G < 2 || a.G > GOAT_NAV_MAX_G || a.G > a.cap + 2 || a.A < 4 || a.A % 4 != 0 || a.A > 64)) return GOAT_E_SHAPE;
  if (t > 0 && (a.Gp < 2 || a.Gp > GOAT_NAV_MAX_G)) return GOAT_E_SHAPE;
  // Layout::small + HDR ints: the R2R lists (<= 11 KB at the limits) and, with objects, the best-object record per node (<= 12 KB at
  // cap = 254, W = 64)
  const size_t lds = (size_t)(Layout(a.cap, T, a.W, a.O).small + HDR) * sizeof(int32_t);
  hipLaunchKernelGGL(nav_step_kernel, dim3(a.B), dim3(256), lds, ST(stream), a);
  GOAT_LAUNCH_CHECK();
  if (t < T) {
    hipLaunchKernelGGL(nav_tail_kernel, dim3(1), dim3(256), 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace

extern "C" int goat_nav_state_ints(int T, int W, int cap) { return nav_sizes_bad(1, T, W, 0, cap, false) ? 0 : Layout(cap, T, W).ints; }
extern "C" int goat_nav_log_ints(int T, int cap) { return nav_sizes_bad(1, T, 1, 0, cap, false) ? 0 : Layout(cap, T, 1).log_ints; }

extern "C" int goat_nav_reset(void* stream, const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B,
                              int T, int W, int cap) {
  return nav_reset(stream, nav_args(scan_tab, si, sd, log, B, T, W, 0, cap), ep, false);
}

extern "C" int goat_nav_step(void* stream, const int64_t* scan_tab, const int64_t* step_tab, int32_t* si, double* sd, int32_t* log,
                             int32_t* ws, const void* act, const double* u, int mode, int t, int B, int T, int G_prev, int G, int W, int A,
                             int cap, int64_t ignoreid) {
  return nav_step(stream, nav_args(scan_tab, si, sd, log, B, T, W, 0, cap, t, ignoreid, step_tab, ws, act, u, mode, G_prev, G, A), false);
}

// goat_nav_obj_*: the same two kernels over a REVERIE / SOON walk.  Args::O > 0 turns on the places where EpisodePlanner.build_step
// branches on its objects: the panorama is W views + O object slots wide, the pool stride of the node embeddings follows it, the
// object tables of the step are written beside the 21 others, [MEM] stays selectable, and an argmax walk records the best object
// of every scored node.  One object slot per thread for loc_fts; the tail forms the object CSRs from the same prefix sums.
extern "C" int goat_nav_obj_state_ints(int T, int W, int O, int cap) {
  return nav_sizes_bad(1, T, W, O, cap, true) ? 0 : Layout(cap, T, W, O).ints;
}

extern "C" int goat_nav_obj_reset(void* stream, const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B,
                                  int T, int W, int O, int cap) {
  return nav_reset(stream, nav_args(scan_tab, si, sd, log, B, T, W, O, cap), ep, true);
}

extern "C" int goat_nav_obj_step(void* stream, const int64_t* scan_tab, const int64_t* obj_tab, const int64_t* step_tab,
                                 const int64_t* ostep_tab, int32_t* si, double* sd, int32_t* log, int32_t* ws, const void* act,
                                 const double* u, const int32_t* goal, int mode, int t, int B, int T, int G_prev, int G, int W, int O,
                                 int max_end, int A, int cap, int64_t ignoreid) {
  return nav_step(stream, nav_args(scan_tab, si, sd, log, B, T, W, O, cap, t, ignoreid, step_tab, ws, act, u, mode, G_prev, G, A, obj_tab,
                                   ostep_tab, goal, max_end), true);
}

extern "C" int goat_nav_expert_doubles(int cap, int max_ref) {
  return (nav_sizes_bad(1, 1, 1, 0, cap, false) || max_ref < 1 || max_ref > GOAT_NAV_MAX_REF) ? 0 : expert_doubles(cap, max_ref);
}

extern "C" int goat_nav_ndtw(void* stream, const int64_t* scan_tab, const int64_t* step_tab, int32_t* si, double* sd, int32_t* log,
                             const int32_t* ref, double* xd, int t, int B, int T, int W, int cap, int max_ref, int64_t ignoreid) {
  const Args a = nav_args(scan_tab, si, sd, log, B, T, W, 0, cap, t, ignoreid, step_tab);
  if (const int bad = nav_check(a, false, step_tab && ref && xd)) return bad;
  if (max_ref < 1 || max_ref > GOAT_NAV_MAX_REF || t < 0 || t >= T) return GOAT_E_SHAPE;
  const Expert x = {ref, xd, max_ref};
  hipLaunchKernelGGL(nav_ndtw_kernel, dim3(B), dim3(256), 0, ST(stream), a, x);
  GOAT_LAUNCH_CHECK();
  return 0;
}
