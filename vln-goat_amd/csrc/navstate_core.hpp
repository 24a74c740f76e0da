// The navigator of a policy-driven walk, one episode at a time (csrc/navstate.hip launches it; the comment there says what it
// restates).  Written against a thread index `tid` of `nt` cooperating threads and a `sync` callable, with no HIP type in it: the
// kernels pass threadIdx / blockDim / __syncthreads, and the same text runs as ordinary C++ with (0, 1, no-op).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef NAV_HD
#define NAV_HD
#endif

namespace navstate {

constexpr double NAV_INF = 95959595.0;      // graph_utils.py:45
constexpr int HDR = 32;
// header words of an episode (the first HDR ints of its read-back block)
enum { H_CUR = 0, H_VIEW, H_ENDED, H_JUST, H_N, H_STATUS, H_STATUS_T, H_START, H_GOAL, H_NOLEFT, H_NSCORED, H_LIVE, H_NSLOT, H_VLEN,
       H_NCAND, H_STARTVIEW, H_HOPN, H_BT_START, H_BT_N, H_K, H_SCAN, H_FOLD /* navexpert_core.hpp: 1 + the hops folded into its DTW row */,
       // object walks (Args::O > 0): 1 + the viewpoint of the best stop node at the forced end of an argmax walk (0: never scored), its
       // best-object record (-1: the viewpoint has no objects), and the objects of the current viewpoint clamped to the bucket O
       H_PRED_VP, H_PRED_OBJ, H_OLEN };
enum { ST_OK = 0, ST_MAP = 1, ST_PANO = 2, ST_ACTION = 3, ST_PATH = 4, ST_OBJ = 5 };
enum { MODE_SAMPLE = 0, MODE_ARGMAX = 1, MODE_FORCED = 2 };
enum { KIND_NONE = 0, KIND_SET = 1, KIND_ACC = 2 };
// the static scan tables, in the order of the address table `scan_tab`
enum { SC_POS = 0, SC_CAND_START, SC_CAND_NB, SC_CAND_POINT, SC_CAND_ANG, SC_CAND_LEN, SC_FEATURE_ROW, SC_VP_SCAN, SC_SCAN_OFF, SC_SCAN_N,
       SC_DIST_OFF, SC_DIST, SC_VAF, SC_VIEW_ANG, SC_PRED /* read by navexpert_core.hpp only */, SC_COUNT };
// the tables of one step, in the order of the address table `step_tab`
enum { TB_FEAT_IDX = 0, TB_FEAT_START, TB_LOC_FTS, TB_NAV_TYPES, TB_VIEW_LENS, TB_STEP_IDS, TB_GMAP_POS, TB_PAIR, TB_VISITED, TB_GMASK,
       TB_VP_POS, TB_VP_MASK, TB_VP_NAV, TB_FUSION, TB_TARGET, TB_CSR_IDX, TB_CSR_START, TB_CSR_SCALE, TB_INV_IDX, TB_INV_START, TB_INV_W,
       TB_COUNT };
// the static object tables (navdev.ObjectTables), in the order of the address table `obj_tab`
enum { OB_START = 0, OB_ROW, OB_DIR, OB_BOX, OB_NAME, OB_COUNT };
// the object tables of one step, in the order of the address table `ostep_tab`
enum { OT_OBJ_IDX = 0, OT_OBJ_START, OT_OBJ_LENS, OT_OBJ_NAMES, OT_VP_OBJ, OT_OBJ_TARGET, OT_OCAT_IDX, OT_OCAT_START, OT_OCAT_INV_IDX,
       OT_OCAT_INV_START, OT_COUNT };

struct Layout {      // ints of an episode's private state / of its read-back block; navdev.py asks goat_nav_*_ints for the sizes
  int cap, T, W, acc;
  int o_vp, o_vis, o_step, o_kind, o_nacc, o_ord, o_slot, o_scored, o_iscand, o_acc, o_P, o_rows, o_cnode, o_seg, o_best, o_stk, small, ints;
  int l_hs, l_hops, log_ints;
  // O_: the object bucket of a REVERIE / SOON walk (0: no objects, the layout of an R2R walk word for word)
  NAV_HD Layout(int cap_, int T_, int W_, int O_ = 0) : cap(cap_), T(T_), W(W_), acc(T_ + 1) {
    int o = 0;
    o_vp = o; o += cap;  o_vis = o; o += cap;  o_step = o; o += cap;  o_kind = o; o += cap;  o_nacc = o; o += cap;
    o_ord = o; o += cap;  o_slot = o; o += cap;  o_scored = o; o += cap;  o_iscand = o; o += cap;
    o_rows = o; o += W;  o_cnode = o; o += W;
    o_seg = o; o += cap + 3;
    o_best = o; o += O_ > 0 ? cap : 0;      // argmax walks with objects: the best object of every scored node (-1: it has none)
    small = o;          // everything above is what the serial parts of a step walk over: a kernel may stage it in LDS
    o_acc = o; o += cap * acc;
    o_P = o; o += cap * cap;
    o_stk = o; o += 2 * cap + 2;
    ints = o;
    l_hs = HDR;  l_hops = l_hs + T + 2;  log_ints = l_hops + (T + 1) * cap;
  }
};

// ints of the workspace `ws` of the batch-wide tail (navdev.workspace computes the same numbers): [B + 1] bases of the view rows and of
// the node-embedding tokens, one owner per pool row of the last step, the live count and, with objects, [B + 1] object bases behind it
struct Workspace {
  int fbase, cbase, owner, live_at, obase, ints;
  NAV_HD Workspace(int B, int T, int W, int O = 0) {
    fbase = 0;
    cbase = B + 1;
    owner = 2 * (B + 1);
    live_at = owner + T * (B * (W + O) + B) + B;
    obase = live_at + 1;
    ints = obase + (O > 0 ? B + 1 : 0);
  }
};

struct Args {
  const int64_t* scan_tab;
  const int64_t* step_tab;      // null when t == T
  int32_t* si;
  double* sd;
  int32_t* log;                 // [2 * T * B] actions, alive, then B read-back blocks
  int32_t* ws;                  // workspace of the batch-wide tail
  const void* act;
  const double* u;
  int mode, t, B, T, Gp, G, W, A, cap;
  int64_t ignoreid;
  // object walks (goat_nav_obj_*); all zero: no objects
  const int64_t* obj_tab;
  const int64_t* ostep_tab;     // null when t == T
  const int32_t* goal;          // [B, max_end, 2]: goal viewpoint (-1: padding), index of the target among its objects or -1
  int O, max_end;
};

template <class T> NAV_HD inline const T* scan_ptr(const Args& a, int k) { return reinterpret_cast<const T*>(a.scan_tab[k]); }
template <class T> NAV_HD inline T* step_ptr(const Args& a, int k) { return reinterpret_cast<T*>(a.step_tab[k]); }
template <class T> NAV_HD inline const T* obj_ptr(const Args& a, int k) { return reinterpret_cast<const T*>(a.obj_tab[k]); }
template <class T> NAV_HD inline T* ostep_ptr(const Args& a, int k) { return reinterpret_cast<T*>(a.ostep_tab[k]); }

struct Ep {       // the views of one episode's state
  Layout L;
  int32_t* S;       // the small arrays (offsets below L.small) and, in H, the header: global memory, or a staged copy of both
  int32_t* Sb;      // the episode's block in global memory: node rows, predecessor matrix, path stack
  int32_t* H;
  int32_t* hs;
  int32_t* hops;
  double* D;
  double* score;
  int cap;
  NAV_HD Ep(const Args& a, int b, int32_t* staged = nullptr) : L(a.cap, a.T, a.W, a.O), cap(a.cap) {
    Sb = a.si + (int64_t)b * L.ints;
    int32_t* G = a.log + (int64_t)2 * a.T * a.B + (int64_t)b * L.log_ints;
    S = staged ? staged : Sb;
    H = staged ? staged + L.small : G;
    hs = G + L.l_hs;
    hops = G + L.l_hops;
    D = a.sd + (int64_t)b * ((int64_t)a.cap * a.cap + a.cap);
    score = D + (int64_t)a.cap * a.cap;
  }
  NAV_HD void fail(int code, int t) const {
    if (H[H_STATUS] == ST_OK) {
      H[H_STATUS] = code;
      H[H_STATUS_T] = t;
    }
  }
  NAV_HD int find(int vp) const {
    const int n = H[H_N];
    for (int i = 0; i < n; ++i)
      if (S[L.o_vp + i] == vp) return i;
    return -1;
  }
  NAV_HD int find_or_add(int vp, int t) const {          // FloydGraph._ix / node_positions[vp] = ...: insertion order
    int i = find(vp);
    if (i >= 0) return i;
    const int n = H[H_N];
    if (n >= cap) {
      fail(ST_MAP, t);
      return -1;
    }
    S[L.o_vp + n] = vp;
    H[H_N] = n + 1;
    return n;
  }
};

// FloydGraph.path (navsim.py:152-159; M/models/graph_utils.py:75-88) from node i to node j under the CURRENT _point matrix, iteratively:
// the pending right halves wait on a stack of at most `nstk` entries.  emit(node) is called for every hop in order.  -> hops, or -1.
template <class Emit>
NAV_HD inline int expand_path(const int32_t* P, int cap, int i, int j, int32_t* stk, int nstk, Emit emit) {
  int sp = 0, hops = 0, guard = 0;
  for (;;) {
    if (++guard > 8 * cap + 8) return -1;
    if (i != j) {
      const int k = P[i * cap + j];
      if (k >= 0) {
        if (sp >= nstk) return -1;
        stk[sp++] = k * 256 + j;      // path(k, j) follows path(i, k)
        j = k;
        continue;
      }
      emit(j);
      ++hops;
    }
    if (sp == 0) return hops;
    const int e = stk[--sp];
    i = e / 256;
    j = e % 256;
  }
}

// GraphMap.update_graph (navsim.py:180-189; graph_utils.py:100-111) for the viewpoint the episode stands on.  Collective.
template <class Sync>
NAV_HD inline void update_graph(const Args& a, const Ep& e, int t, int tid, int nt, Sync sync) {
#pragma clang fp contract(off)
  const int cap = e.cap;
  int32_t* P = e.Sb + e.L.o_P;
  if (tid == 0) {
    const int32_t* cs = scan_ptr<int32_t>(a, SC_CAND_START);
    const int32_t* nb = scan_ptr<int32_t>(a, SC_CAND_NB);
    const double* len = scan_ptr<double>(a, SC_CAND_LEN);
    const int v = e.H[H_CUR];
    const int k = e.find_or_add(v, t);
    e.H[H_K] = k;
    if (k >= 0) {
      for (int c = cs[v]; c < cs[v + 1]; ++c) {
        const int j = e.find_or_add(nb[c], t);
        if (j < 0) continue;
        const double d = len[c];
        if (d < e.D[k * cap + j]) {         // FloydGraph.add_edge
          e.D[k * cap + j] = e.D[j * cap + k] = d;
          P[k * cap + j] = P[j * cap + k] = -1;
        }
      }
    }
  }
  sync();
  const int n = e.H[H_N], k = e.H[H_K];
  if (k >= 0) {
    // FloydGraph.update(k): row and column k cannot improve (D[k][k] keeps the default), so the relaxation reads nothing it writes
    for (int x = tid; x < n * n; x += nt) {
      const int i = x / n, j = x % n;
      if (i == j) continue;
      const double c = e.D[i * cap + k] + e.D[k * cap + j];
      if (c < e.D[i * cap + j]) {
        e.D[i * cap + j] = c;
        P[i * cap + j] = k;
      }
    }
    if (tid == 0) e.S[e.L.o_vis + k] = 1;
  }
  sync();
}

// start_walk (nav_inputs.py:223-230): a fresh map, the first update_graph.  Collective.
template <class Sync>
NAV_HD inline void reset_episode(const Args& a, const int32_t* ep, int b, int tid, int nt, Sync sync) {
  Ep e(a, b);
  const int cap = a.cap;
  for (int x = tid; x < e.L.ints; x += nt) e.S[x] = (x >= e.L.o_P && x < e.L.o_P + cap * cap) ? -1 : 0;
  for (int x = tid; x < cap * cap + cap; x += nt) e.D[x] = x < cap * cap ? NAV_INF : 0.0;
  for (int x = tid; x < e.L.log_ints; x += nt) e.H[x] = 0;
  for (int x = tid; x < 2 * a.T; x += nt) a.log[(int64_t)x * a.B + b] = 0;
  sync();
  if (tid == 0) {
    e.H[H_SCAN] = ep[b * 4 + 0];
    e.H[H_CUR] = e.H[H_START] = ep[b * 4 + 1];
    e.H[H_VIEW] = e.H[H_STARTVIEW] = ep[b * 4 + 2];
    e.H[H_GOAL] = ep[b * 4 + 3];
  }
  sync();
  update_graph(a, e, 0, tid, nt, sync);
}

NAV_HD inline double toward_zero(double c) {        // numpy.nextafter(c, 0.0)
  if (c == 0.0 || c != c) return c;
  int64_t bits;
  memcpy(&bits, &c, 8);
  bits -= 1;
  memcpy(&c, &bits, 8);
  return c;
}

// The action of step tp in the mode of the walk; an episode that has ended stops.  Thread 0.
NAV_HD inline int mode_action(const Args& a, int b, int tp, int ended) {
#pragma clang fp contract(off)
  if (a.mode == MODE_SAMPLE) {           // SampledEpisode.sample (sampled.py:115-121): float64 cumulative sum in slot order
    const float* p = reinterpret_cast<const float*>(a.act) + (int64_t)b * a.Gp;
    double total = 0.0;
    for (int g = 0; g < a.Gp; ++g) total = total + (double)p[g];
    const double lim = toward_zero(total);
    double x = a.u[(int64_t)tp * a.B + b] * total;
    if (lim < x) x = lim;
    double c = 0.0;
    int act = a.Gp;
    for (int g = 0; g < a.Gp; ++g) {
      c = c + (double)p[g];
      if (c > x) {
        act = g;
        break;
      }
    }
    return ended ? 0 : act;
  }
  if (a.mode == MODE_ARGMAX) return ended ? 0 : (int)reinterpret_cast<const float*>(a.act)[b];
  return reinterpret_cast<const int32_t*>(a.act)[(int64_t)tp * a.B + b];
}

// node_stop_scores[viewpoint] = {'stop': score} of an argmax walk for the viewpoint `cur` the live episode stands on.  Thread 0.
NAV_HD inline void record_stop_score(const Args& a, const Ep& e, int b, int cur) {
  const float* back = reinterpret_cast<const float*>(a.act);
  const int ci = e.find(cur);
  if (ci < 0) return;
  bool seen = false;
  for (int i = 0; i < e.H[H_NSCORED]; ++i) seen = seen || e.S[e.L.o_scored + i] == ci;
  if (!seen) e.S[e.L.o_scored + e.H[H_NSCORED]++] = ci;
  e.score[ci] = (double)back[a.B + b];
  // ['og'] = obj_ids[best object] | None: row 2 is read only where the viewpoint has objects (elsewhere it holds the argmax
  // of an all -inf row less v + 2, a negative number)
  if (a.O > 0) e.S[e.L.o_best + ci] = e.H[H_OLEN] > 0 ? (int)back[2 * a.B + b] : -1;
}

// FloydGraph.path from node `from` (-1: the viewpoint is not in the map) to node `to`, its viewpoints logged behind the `hopn` hops the
// walk has made -> hops; 0 with the status word set where there is no path or the hop log has no room for it.  Thread 0.
NAV_HD inline int log_path(const Args& a, const Ep& e, int tp, int from, int to, int hopn) {
  const int cap = a.cap, room = (a.T + 1) * cap - hopn;
  int wrote = 0;
  int32_t* out = e.hops + hopn;
  const int32_t* vp = e.S + e.L.o_vp;
  const int n = from < 0 ? -1 : expand_path(e.Sb + e.L.o_P, cap, from, to, e.Sb + e.L.o_stk, 2 * cap + 2, [&](int node) {
    if (wrote < room) out[wrote] = vp[node];
    ++wrote;
  });
  if (n >= 1 && wrote <= room) return n;
  e.fail(ST_PATH, tp);
  return 0;
}

// EpisodePlanner.advance of step tp (episodes.py:300-357) with the action of the mode.  Collective.
template <class Sync>
NAV_HD inline void advance_episode(const Args& a, const Ep& e, int b, int tp, int tid, int nt, Sync sync) {
#pragma clang fp contract(off)
  const int ended = e.H[H_ENDED];
  sync();
  if (tid == 0) {
    const int cur = e.H[H_CUR];
    const bool argmax = a.mode == MODE_ARGMAX;
    const int act = mode_action(a, b, tp, ended);
    if (argmax && !ended) record_stop_score(a, e, b, cur);
    a.log[(int64_t)tp * a.B + b] = act;
    a.log[(int64_t)(a.T + tp) * a.B + b] = !ended;
    const bool stop = argmax ? act == 0 : cur == e.H[H_GOAL];
    int dest = -1, view = e.H[H_VIEW];
    int hopn = e.H[H_HOPN];
    if (stop || ended || e.H[H_NOLEFT] || tp == a.T - 1) {
      if (argmax) e.H[H_JUST] = 1;
    } else {
      const int nslots = e.H[H_NSLOT];
      if (act < 0 || act >= nslots || act == 1 || (act > 1 && e.S[e.L.o_vis + e.S[e.L.o_ord + act - 2]])) {
        e.fail(ST_ACTION, tp);                 // the host planner raises here; the walk goes on as if the episode had stopped
      } else if (act >= 2) {
        const int dn = e.S[e.L.o_ord + act - 2];
        const int n = log_path(a, e, tp, e.find(cur), dn, hopn);
        if (n > 0) {
          dest = e.S[e.L.o_vp + dn];
          const int prev = n == 1 ? cur : e.hops[hopn + n - 2];
          const int32_t* cs = scan_ptr<int32_t>(a, SC_CAND_START);
          const int32_t* nb = scan_ptr<int32_t>(a, SC_CAND_NB);
          const int32_t* pt = scan_ptr<int32_t>(a, SC_CAND_POINT);
          bool found = false;
          for (int c = cs[prev]; c < cs[prev + 1] && !found; ++c)
            if (nb[c] == dest) {
              view = pt[c];
              found = true;
            }
          if (!found) e.fail(ST_PATH, tp);
          hopn += n;
        }
      }
    }
    e.hs[tp + 1] = ended ? e.hs[tp] : hopn;       // (the backtrack's hops lie behind the last move's: no step owns them)
    if (argmax && !ended && e.H[H_JUST] && e.H[H_NSCORED] > 0) {       // back to the best stop node: the first maximum in visit order
      int best = e.S[e.L.o_scored];
      for (int i = 1; i < e.H[H_NSCORED]; ++i) {
        const int c = e.S[e.L.o_scored + i];
        if (e.score[c] > e.score[best]) best = c;
      }
      if (a.O > 0) {                        // traj['pred_objid'] = score.get('og')
        e.H[H_PRED_VP] = e.S[e.L.o_vp + best] + 1;
        e.H[H_PRED_OBJ] = e.S[e.L.o_best + best];
      }
      const int ci = e.find(cur);
      if (ci >= 0 && best != ci) {
        const int n = log_path(a, e, tp, ci, best, hopn);
        if (n > 0) {
          e.H[H_BT_START] = hopn;
          e.H[H_BT_N] = n;
          hopn += n;
        }
      }
    }
    e.H[H_HOPN] = hopn;
    if (dest >= 0) {
      e.H[H_CUR] = dest;
      e.H[H_VIEW] = view;
    }
    e.H[H_K] = dest;
  }
  sync();
  const int moved = e.H[H_K] >= 0;
  sync();
  if (!ended) update_graph(a, e, tp, tid, nt, sync);
  if (tid == 0) e.H[H_ENDED] = ended || !moved;
  sync();
}

NAV_HD inline void angle_row(float* out, int A, double h, double el) {        // navsim.angle_feature
  const float f[4] = {(float)sin(h), (float)cos(h), (float)sin(el), (float)cos(el)};
  for (int x = 0; x < A; ++x) out[x] = f[x % 4];
}

// The serial jobs of EpisodePlanner.build_step of step a.t (episodes.py:245-298) for one episode, in its order.  Thread 0.

// panorama_inputs: the candidates' views, then the views no candidate used; with objects, the viewpoint's count clamped to the bucket
NAV_HD inline void pano_order(const Args& a, const Ep& e, int b) {
  const int W = a.W, O = a.O, t = a.t, cur = e.H[H_CUR];
  const Layout& L = e.L;
  int32_t* S = e.S;
  const int32_t* cs = scan_ptr<int32_t>(a, SC_CAND_START);
  const int32_t* pt = scan_ptr<int32_t>(a, SC_CAND_POINT);
  const int c0 = cs[cur];
  const int fr = scan_ptr<int32_t>(a, SC_FEATURE_ROW)[cur];
  const int ncand = cs[cur + 1] - c0;
  uint64_t used = 0;
  int len = 0;
  for (int c = 0; c < ncand; ++c) {
    if (len < W) S[L.o_rows + len] = fr * 36 + pt[c0 + c];
    used |= (uint64_t)1 << pt[c0 + c];
    ++len;
  }
  for (int k = 0; k < 36; ++k)
    if (!((used >> k) & 1)) {
      if (len < W) S[L.o_rows + len] = fr * 36 + k;
      ++len;
    }
  if (len > W) {
    e.fail(ST_PANO, t);
    len = W;
  }
  e.H[H_VLEN] = len;
  e.H[H_NCAND] = ncand < W ? ncand : W;
  step_ptr<int64_t>(a, TB_VIEW_LENS)[b] = len;
  if (O > 0) {      // the objects of the viewpoint: contiguous rows of ObjectStore.table
    const int32_t* os = obj_ptr<int32_t>(a, OB_START);
    int olen = os[cur + 1] - os[cur];
    if (olen > O) {
      e.fail(ST_OBJ, t);
      olen = O;
    }
    e.H[H_OLEN] = olen;
    ostep_ptr<int64_t>(a, OT_OBJ_LENS)[b] = olen;
  }
}

// note_step (nav_inputs.py:233-243)
NAV_HD inline void note_step(const Args& a, const Ep& e, int b) {
  const int t = a.t, B = a.B, WT = a.W + a.O, ended = e.H[H_ENDED], cur = e.H[H_CUR], n = e.H[H_N];
  const int view_base = t * (B * WT + B), fused_base = view_base + B * WT;      // store.advance(B, te.WT)
  const Layout& L = e.L;
  int32_t* S = e.S;
  const int32_t* nb = scan_ptr<int32_t>(a, SC_CAND_NB);
  const int c0 = scan_ptr<int32_t>(a, SC_CAND_START)[cur];
  for (int i = 0; i < n; ++i) S[L.o_iscand + i] = 0;
  const int ci = e.find(cur);
  if (!ended && ci >= 0) {
    S[L.o_step + ci] = t + 1;
    S[L.o_kind + ci] = KIND_SET;
    S[L.o_nacc + ci] = 1;
    e.Sb[L.o_acc + ci * L.acc] = fused_base + b;
  }
  for (int c = 0; c < e.H[H_NCAND]; ++c) {
    const int j = e.find(nb[c0 + c]);
    S[L.o_cnode + c] = j;
    if (j < 0) continue;
    S[L.o_iscand + j] = 1;
    if (!ended && !S[L.o_vis + j]) {            // NodeEmbedStore.accumulate
      const int row = view_base + b * WT + c;
      int32_t* acc = e.Sb + L.o_acc + j * L.acc;
      if (S[L.o_kind + j] == KIND_NONE) {
        S[L.o_kind + j] = KIND_ACC;
        S[L.o_nacc + j] = 1;
        acc[0] = row;
      } else if (S[L.o_nacc + j] < L.acc) {
        S[L.o_kind + j] = KIND_ACC;
        acc[S[L.o_nacc + j]++] = row;
      } else {
        e.fail(ST_PATH, t);
      }
    }
  }
}

// gmap_order: [stop], [MEM], the visited nodes, the unvisited ones, each in insertion order; behind note_step, the episode's share of the
// node-embedding CSR
NAV_HD inline void map_order(const Args& a, const Ep& e) {
  const int t = a.t, G = a.G, n = e.H[H_N];
  const Layout& L = e.L;
  int32_t* S = e.S;
  int nv = 0;
  for (int i = 0; i < n; ++i)
    if (S[L.o_vis + i]) S[L.o_ord + nv++] = i;
  int nu = nv;
  for (int i = 0; i < n; ++i)
    if (!S[L.o_vis + i]) S[L.o_ord + nu++] = i;
  for (int k = 0; k < n; ++k) S[L.o_slot + S[L.o_ord + k]] = k + 2;
  e.H[H_NOLEFT] = nu == nv;
  int nslots = n + 2;
  if (nslots > G) {
    e.fail(ST_MAP, t);
    nslots = G;
  }
  e.H[H_NSLOT] = nslots;
  // the episode's share of the node-embedding CSR (NodeEmbedStore.csr): tokens per slot as a running sum
  int tok = 0;
  S[L.o_seg] = 0;
  for (int g = 0; g < G; ++g) {
    int cnt = 0;
    if (g == 1 && t > 0) cnt = 1;
    else if (g >= 2 && g < nslots) cnt = S[L.o_nacc + S[L.o_ord + g - 2]];
    tok += cnt;
    S[L.o_seg + g + 1] = tok;
  }
}

// the two DAgger labels of the step: the node to move to and, with objects, the object to pick
NAV_HD inline void teacher_labels(const Args& a, const Ep& e, int b) {
#pragma clang fp contract(off)
  const int ended = e.H[H_ENDED], cur = e.H[H_CUR], nslots = e.H[H_NSLOT];
  const Layout& L = e.L;
  const int32_t* S = e.S;
  // teacher_action(imitation_learning=False) (nav_inputs.py:205-218): strict <, the first minimum wins
  int64_t target = a.ignoreid;
  if (!ended) {
    const int goal = e.H[H_GOAL];
    if (cur == goal) {
      target = 0;
    } else {
      const int s = e.H[H_SCAN];
      const int off = scan_ptr<int32_t>(a, SC_SCAN_OFF)[s], ns = scan_ptr<int32_t>(a, SC_SCAN_N)[s];
      const double* dist = scan_ptr<double>(a, SC_DIST) + scan_ptr<int64_t>(a, SC_DIST_OFF)[s];
      double best = INFINITY;
      for (int g = 2; g < nslots; ++g) {
        const int node = S[L.o_ord + g - 2];
        if (S[L.o_vis + node]) continue;
        const int k = S[L.o_vp + node] - off;
        const double d = dist[(int64_t)k * ns + (goal - off)] + dist[(int64_t)(cur - off) * ns + k];
        if (d < best) {
          best = d;
          target = g;
        }
      }
    }
  }
  step_ptr<int64_t>(a, TB_TARGET)[b] = target;
  if (a.O > 0) {
    // teacher_object (nav_inputs.py:175-186): on one of the episode's end viewpoints the slot of the target object among [stop],
    // [MEM], the views and the objects; the ignore value elsewhere and where the target is not among the viewpoint's objects
    const int olen = e.H[H_OLEN], len = e.H[H_VLEN];
    int64_t ot = a.ignoreid;
    if (!ended) {
      const int32_t* goal = a.goal + (int64_t)b * a.max_end * 2;
      for (int k = 0; k < a.max_end; ++k)
        if (goal[2 * k] == cur) {         // (a viewpoint listed twice carries the same index)
          const int j = goal[2 * k + 1];
          if (j >= 0 && j < olen) ot = j + len + 2;
          break;
        }
    }
    ostep_ptr<int64_t>(a, OT_OBJ_TARGET)[b] = ot;
  }
}

// The token tables of the step, spread over the threads.  bh, be: heading and elevation of the view the episode looks along.

// panorama tokens (panorama_inputs / panorama_object_inputs, vp_inputs' masks)
NAV_HD inline void pano_tokens(const Args& a, const Ep& e, int b, double bh, double be, int tid, int nt) {
#pragma clang fp contract(off)
  const int W = a.W, A = a.A, C = a.A + 3;
  const int O = a.O, WT = W + O;        // object walks: O object slots behind the W views of every panorama (panorama_object_inputs)
  const Layout& L = e.L;
  const int32_t* S = e.S;
  const int cur = e.H[H_CUR], view = e.H[H_VIEW], vlen = e.H[H_VLEN], ncand = e.H[H_NCAND];
  const int c0 = scan_ptr<int32_t>(a, SC_CAND_START)[cur];
  const double* cang = scan_ptr<double>(a, SC_CAND_ANG);
  const float* vaf = scan_ptr<float>(a, SC_VAF);
  const int fr36 = scan_ptr<int32_t>(a, SC_FEATURE_ROW)[cur] * 36;
  float* loc = step_ptr<float>(a, TB_LOC_FTS) + (int64_t)b * WT * C;
  int64_t* ty = step_ptr<int64_t>(a, TB_NAV_TYPES) + (int64_t)b * WT;
  uint8_t* vm = step_ptr<uint8_t>(a, TB_VP_MASK) + (int64_t)b * (WT + 2);
  uint8_t* vn = step_ptr<uint8_t>(a, TB_VP_NAV) + (int64_t)b * (WT + 2);
  const int olen = O > 0 ? e.H[H_OLEN] : 0;
  const int o0 = O > 0 ? obj_ptr<int32_t>(a, OB_START)[cur] : 0;
  for (int j = tid; j < WT; j += nt) {
    float* row = loc + j * C;
    if (j >= vlen && j < vlen + olen) {
      // ObjectStore.attributes: the object tokens follow the views (nav type 2): [angle_feature(direction - base) | box]
      const double* dir = obj_ptr<double>(a, OB_DIR) + (int64_t)(o0 + j - vlen) * 2;
      const float* box = obj_ptr<float>(a, OB_BOX) + (int64_t)(o0 + j - vlen) * 3;
      angle_row(row, A, dir[0] - bh, dir[1] - be);
      for (int x = 0; x < 3; ++x) row[A + x] = box[x];
      ty[j] = 2;
      continue;
    }
    if (j < ncand) {
      angle_row(row, A, cang[(c0 + j) * 2] - bh, cang[(c0 + j) * 2 + 1] - be);
    } else if (j < vlen) {
      const float* src = vaf + ((int64_t)view * 36 + (S[L.o_rows + j] - fr36)) * A;
      for (int x = 0; x < A; ++x) row[x] = src[x];
    } else {
      for (int x = 0; x < A; ++x) row[x] = 0.0f;
    }
    for (int x = A; x < C; ++x) row[x] = j < vlen ? 1.0f : 0.0f;
    ty[j] = j < ncand ? 1 : 0;
  }
  for (int j = tid; j < WT + 2; j += nt) {
    vm[j] = j < vlen + olen + 2;
    vn[j] = j == 0 ? 1 : (j == 1 ? 0 : (j - 2 < ncand));
  }
  if (O > 0) {
    uint8_t* vo = ostep_ptr<uint8_t>(a, OT_VP_OBJ) + (int64_t)b * (WT + 2);
    int64_t* names = ostep_ptr<int64_t>(a, OT_OBJ_NAMES) + (int64_t)b * O;
    const int64_t* name = obj_ptr<int64_t>(a, OB_NAME);
    // vp_inputs: the head of vp_nav_masks ([stop] true, [MEM] false), then nav_types == 2
    for (int j = tid; j < WT + 2; j += nt) vo[j] = j == 0 ? 1 : (j - 2 >= vlen && j - 2 < vlen + olen);
    for (int j = tid; j < O; j += nt) names[j] = j < olen ? name[o0 + j] : 0;
  }
}

// map tokens (gmap_inputs, GraphMap.get_pos_fts / pair_dists) and the logit fusion matrix
NAV_HD inline void map_tokens(const Args& a, const Ep& e, int b, double bh, double be, int tid, int nt) {
#pragma clang fp contract(off)
  const int cap = a.cap, G = a.G, A = a.A, C = a.A + 3, O = a.O, WT = a.W + a.O;
  const Layout& L = e.L;
  const int32_t* S = e.S;
  const int cur = e.H[H_CUR], ncand = e.H[H_NCAND], nslots = e.H[H_NSLOT];
  const double* pos = scan_ptr<double>(a, SC_POS);
  const int32_t* P = e.Sb + L.o_P;
  int64_t* sid = step_ptr<int64_t>(a, TB_STEP_IDS) + (int64_t)b * G;
  uint8_t* vmask = step_ptr<uint8_t>(a, TB_VISITED) + (int64_t)b * G;
  uint8_t* gmask = step_ptr<uint8_t>(a, TB_GMASK) + (int64_t)b * G;
  float* scale = step_ptr<float>(a, TB_CSR_SCALE) + (int64_t)b * G;
  float* gp = step_ptr<float>(a, TB_GMAP_POS) + (int64_t)b * G * C;
  const int ci = e.find(cur);
  const double ax = pos[cur * 3], ay = pos[cur * 3 + 1], az = pos[cur * 3 + 2];
  for (int g = tid; g < G; g += nt) {
    float* row = gp + g * C;
    const bool real = g >= 2 && g < nslots;
    const int node = real ? S[L.o_ord + g - 2] : -1;
    sid[g] = real ? S[L.o_step + node] : 0;
    vmask[g] = g == 1 ? 1 : (real ? S[L.o_vis + node] != 0 : 0);
    gmask[g] = g < nslots && (g != 1 || O > 0);      // (gmap_inputs(mem_selectable=has_obj): the REVERIE builder keeps [MEM])
    scale[g] = (real && S[L.o_kind + node] == KIND_ACC) ? (float)(1.0 / (double)S[L.o_nacc + node]) : 1.0f;
    if (g >= nslots) {
      for (int x = 0; x < C; ++x) row[x] = 0.0f;
      continue;
    }
    float h32 = 0.0f, e32 = 0.0f;
    double line = 0.0, md = 0.0, hops = 0.0;
    if (real) {
      const int v = S[L.o_vp + node];
      const double by = pos[v * 3 + 1];
      const double dx = pos[v * 3] - ax, dy = by - ay, dz = pos[v * 3 + 2] - az;       // navsim.rel_pos
      const double xy = fmax(sqrt(dx * dx + dy * dy), 1e-8);
      const double xyz = fmax(sqrt(dx * dx + dy * dy + dz * dz), 1e-8);
      double hd = asin(dx / xy);
      if (by < ay) hd = 3.141592653589793 - hd;
      const double el = asin(dz / xyz);
      h32 = (float)(hd - bh);
      e32 = (float)(el - be);
      line = xyz / 30.0;
      if (ci >= 0 && node != ci) {
        md = e.D[ci * cap + node] / 30.0;
        int32_t stk[256];
        const int nh = expand_path(P, cap, ci, node, stk, 256, [](int) {});
        hops = (double)(nh < 0 ? 0 : nh) / 10.0;
      }
    }
    // get_angle_fts: sin / cos of the float32 angles
    const float f[4] = {(float)sin((double)h32), (float)cos((double)h32), (float)sin((double)e32), (float)cos((double)e32)};
    for (int x = 0; x < A; ++x) row[x] = f[x % 4];
    row[A] = (float)line;
    row[A + 1] = (float)md;
    row[A + 2] = (float)hops;
  }
  float* pair = step_ptr<float>(a, TB_PAIR) + (int64_t)b * G * G;
  for (int x = tid; x < G * G; x += nt) {
    const int g = x / G, h = x % G;
    float v = 0.0f;
    if (g >= 2 && h >= 2 && g < nslots && h < nslots && g != h) v = (float)e.D[S[L.o_ord + g - 2] * cap + S[L.o_ord + h - 2]];
    pair[x] = v;
  }
  // nav_fusion_matrix (nav_model.py:231-253)
  float* fus = step_ptr<float>(a, TB_FUSION) + (int64_t)b * G * (WT + 2);
  for (int x = tid; x < G * (WT + 2); x += nt) {
    const int g = x / (WT + 2), j = x % (WT + 2);
    float v = 0.0f;
    if (g >= 2 && g < nslots && j >= 2 && j - 2 < ncand) {
      const int node = S[L.o_ord + g - 2], cn = S[L.o_cnode + j - 2];
      if (!S[L.o_vis + node] && cn >= 0) {
        if (cn == node) v = 1.0f;
        else if (S[L.o_vis + cn] && !S[L.o_iscand + node]) v = 1.0f;
      }
    }
    fus[x] = v;
  }
}

// vp_inputs: the start node's row in every slot, the candidates' rows behind it (rows of gmap_pos_fts, all of them written)
NAV_HD inline void vp_tokens(const Args& a, const Ep& e, int b, int tid, int nt) {
  const int G = a.G, C = a.A + 3, WT = a.W + a.O;
  const Layout& L = e.L;
  const int32_t* S = e.S;
  const int ncand = e.H[H_NCAND], nslots = e.H[H_NSLOT];
  const float* gp = step_ptr<float>(a, TB_GMAP_POS) + (int64_t)b * G * C;
  float* vp = step_ptr<float>(a, TB_VP_POS) + (int64_t)b * (WT + 2) * 2 * C;
  const int sn = e.find(e.H[H_START]);
  const int sslot = sn >= 0 ? S[L.o_slot + sn] : G;
  for (int x = tid; x < (WT + 2) * 2 * C; x += nt) {
    const int j = x / (2 * C), c = x % (2 * C);
    float v = 0.0f;
    if (c < C) {
      if (sslot < nslots) v = gp[sslot * C + c];
    } else if (j >= 2 && j - 2 < ncand) {
      const int cn = S[L.o_cnode + j - 2];
      const int slot = cn >= 0 ? S[L.o_slot + cn] : G;
      if (slot < nslots) v = gp[slot * C + c - C];
    }
    vp[x] = v;
  }
}

// EpisodePlanner.build_step of step t (episodes.py:245-298) for one episode: every table row of the episode except the batch-wide
// compact CSRs, whose pieces it leaves in the state for nav_tail.  Collective.
template <class Sync>
NAV_HD inline void build_episode(const Args& a, const Ep& e, int b, int tid, int nt, Sync sync) {
  if (tid == 0) {
    if (!e.H[H_ENDED]) e.H[H_LIVE] += 1;
    pano_order(a, e, b);
    note_step(a, e, b);
    map_order(a, e);
    teacher_labels(a, e, b);
  }
  sync();
  const double* vang = scan_ptr<double>(a, SC_VIEW_ANG);
  const double bh = vang[e.H[H_VIEW] * 2], be = vang[e.H[H_VIEW] * 2 + 1];
  pano_tokens(a, e, b, bh, be, tid, nt);
  map_tokens(a, e, b, bh, be, tid, nt);
  sync();
  vp_tokens(a, e, b, tid, nt);
}

// One step of one episode: the move of step t - 1, then the tables of step t.
template <class Sync>
NAV_HD inline void step_episode(const Args& a, int b, int tid, int nt, Sync sync, int32_t* staged = nullptr) {
  // staged: room for Layout::small + HDR ints all threads share (LDS).  The serial parts are chains of dependent loads over the node
  // lists; from LDS each costs a fraction of a trip to L2.
  Ep e(a, b, staged);
  if (staged) {
    Ep g(a, b);
    for (int x = tid; x < e.L.small; x += nt) staged[x] = g.S[x];
    for (int x = tid; x < HDR; x += nt) e.H[x] = g.H[x];
    sync();
  }
  if (a.t > 0) advance_episode(a, e, b, a.t - 1, tid, nt, sync);
  if (a.t < a.T) build_episode(a, e, b, tid, nt, sync);
  if (staged) {
    Ep g(a, b);
    sync();
    for (int x = tid; x < e.L.small; x += nt) g.S[x] = staged[x];
    for (int x = tid; x < HDR; x += nt) g.H[x] = e.H[x];
  }
}

// episodes.py:_compact_rows for slot s of a [B, width] table: row j of an episode whose `len` real rows lie from `base` on.  The slot's
// start, the index `row` of a real row where it lands, and -1 in idx behind the `total` rows of the batch (NO_FILL: the caller's).  -> there
constexpr int NO_FILL = 0x7fffffff;
NAV_HD inline int compact_row(int32_t* start, int32_t* idx, int s, int base, int j, int len, int row, int total) {
  const int at = base + (j < len ? j : len);
  start[s] = at;
  if (j < len) idx[at] = row;
  if (s >= total) idx[s] = -1;
  return at;
}

// The batch-wide tail of a step: the compact CSRs are prefix sums over the episodes (episodes.py:_compact_rows, NodeEmbedStore.csr,
// graphmap.inverse_index).  One group of threads; `part` holds nt ints they share.  ws: the ints of Workspace.
template <class Sync>
NAV_HD inline void nav_tail(const Args& a, int32_t* part, int tid, int nt, Sync sync) {
  const int B = a.B, G = a.G, W = a.W, t = a.t, O = a.O, WT = a.W + a.O;
  const int rows = (t + 1) * (B * WT + B), n_src = rows + (t > 0 ? B : 0);
  const Workspace ws(B, a.T, W, O);
  int32_t* obase = a.ws + ws.obase;      // object walks: [B + 1] behind the live count
  int32_t* fbase = a.ws + ws.fbase;
  int32_t* cbase = a.ws + ws.cbase;
  int32_t* owner = a.ws + ws.owner;
  int32_t* feat_idx = step_ptr<int32_t>(a, TB_FEAT_IDX);
  int32_t* feat_start = step_ptr<int32_t>(a, TB_FEAT_START);
  int32_t* csr_idx = step_ptr<int32_t>(a, TB_CSR_IDX);
  int32_t* csr_start = step_ptr<int32_t>(a, TB_CSR_START);
  const float* csr_scale = step_ptr<float>(a, TB_CSR_SCALE);
  int32_t* inv_idx = step_ptr<int32_t>(a, TB_INV_IDX);
  int32_t* inv_start = step_ptr<int32_t>(a, TB_INV_START);
  float* inv_w = step_ptr<float>(a, TB_INV_W);
  if (tid == 0) {
    int f = 0, c = 0, live = 0, o = 0;
    for (int b = 0; b < B; ++b) {
      Ep e(a, b);
      fbase[b] = f;
      cbase[b] = c;
      if (O > 0) {
        obase[b] = o;
        o += e.H[H_OLEN];
      }
      f += e.H[H_VLEN];
      c += e.S[e.L.o_seg + G];
      live += !e.H[H_ENDED];
    }
    fbase[B] = f;
    cbase[B] = c;
    if (O > 0) obase[B] = o;
    a.ws[ws.live_at] = live;      // episodes still walking when step t begins (an optional host read)
  }
  for (int r = tid; r < n_src; r += nt) owner[r] = -1;
  sync();
  const int ftot = fbase[B], ctot = cbase[B];
  for (int s = tid; s < B * W; s += nt) {
    const int b = s / W, j = s % W;
    Ep e(a, b);
    compact_row(feat_start, feat_idx, s, fbase[b], j, e.H[H_VLEN], e.S[e.L.o_rows + j], ftot);
  }
  if (tid == 0) {
    feat_start[B * W] = ftot;
    csr_start[B * G] = ctot;
    inv_start[n_src] = ctot;
  }
  if (O > 0) {
    // _compact_rows(obj_rows) and _obj_concat_tables (graphmap.build_obj_concat_index / inverse_index): token J of panorama b is view J
    // (source row b * W + J) or object J - view_len (source row B * W + b * O + J - view_len).  A source row is read by at most one
    // token and the tokens of a panorama read ascending rows, so the inverse lists the views of all panoramas, then their objects.
    const int32_t* orow = obj_ptr<int32_t>(a, OB_ROW);
    int32_t* obj_idx = ostep_ptr<int32_t>(a, OT_OBJ_IDX);
    int32_t* obj_start = ostep_ptr<int32_t>(a, OT_OBJ_START);
    int32_t* cat_idx = ostep_ptr<int32_t>(a, OT_OCAT_IDX);
    int32_t* cat_start = ostep_ptr<int32_t>(a, OT_OCAT_START);
    int32_t* cinv_idx = ostep_ptr<int32_t>(a, OT_OCAT_INV_IDX);
    int32_t* cinv_start = ostep_ptr<int32_t>(a, OT_OCAT_INV_START);
    const int otot = obase[B], ttot = ftot + otot;
    for (int s = tid; s < B * O; s += nt) {
      const int b = s / O, j = s % O;
      Ep e(a, b);
      const int ol = e.H[H_OLEN];
      compact_row(obj_start, obj_idx, s, obase[b], j, ol, orow[e.H[H_CUR]] + j, otot);
      compact_row(cinv_start + B * W, cinv_idx, s, ftot + obase[b], j, ol, b * WT + e.H[H_VLEN] + j, NO_FILL);
    }
    for (int s = tid; s < B * W; s += nt) {
      const int b = s / W, j = s % W;
      Ep e(a, b);
      compact_row(cinv_start, cinv_idx, s, fbase[b], j, e.H[H_VLEN], b * WT + j, NO_FILL);
    }
    for (int s = tid; s < B * WT; s += nt) {
      const int b = s / WT, j = s % WT;
      Ep e(a, b);
      const int vl = e.H[H_VLEN];
      compact_row(cat_start, cat_idx, s, fbase[b] + obase[b], j, vl + e.H[H_OLEN], j < vl ? b * W + j : B * W + b * O + (j - vl), ttot);
      if (s >= ttot) cinv_idx[s] = -1;
    }
    if (tid == 0) {
      obj_start[B * O] = otot;
      cat_start[B * WT] = ttot;
      cinv_start[B * W + B * O] = ttot;
    }
  }
  for (int s = tid; s < B * G; s += nt) {
    const int b = s / G, g = s % G;
    Ep e(a, b);
    const int lo = e.S[e.L.o_seg + g], cnt = e.S[e.L.o_seg + g + 1] - lo, at = cbase[b] + lo;
    csr_start[s] = at;
    if (cnt == 0) continue;
    if (g == 1) {
      csr_idx[at] = rows + b;
      owner[rows + b] = s;
    } else {
      const int32_t* acc = e.S + e.L.o_acc + e.S[e.L.o_ord + g - 2] * e.L.acc;
      for (int i = 0; i < cnt; ++i) {
        const int r = acc[i];
        csr_idx[at + i] = r;
        if (r >= 0 && r < n_src) owner[r] = s;
      }
    }
  }
  for (int s = ctot + tid; s < n_src; s += nt) {
    csr_idx[s] = -1;
    inv_idx[s] = -1;
    inv_w[s] = 0.0f;
  }
  sync();
  // inverse index: a pool row is read by at most one segment, so "grouped by source row" is the order of the rows themselves
  const int chunk = (n_src + nt - 1) / nt;
  const int lo = tid * chunk < n_src ? tid * chunk : n_src, hi = lo + chunk < n_src ? lo + chunk : n_src;
  int cnt = 0;
  for (int r = lo; r < hi; ++r) cnt += owner[r] >= 0;
  part[tid] = cnt;
  sync();
  int at = 0;
  for (int i = 0; i < tid; ++i) at += part[i];
  for (int r = lo; r < hi; ++r) {
    inv_start[r] = at;
    const int s = owner[r];
    if (s >= 0 && at < n_src) {
      inv_idx[at] = s;
      inv_w[at] = csr_scale[s];
      ++at;
    }
  }
}

}  // namespace navstate
