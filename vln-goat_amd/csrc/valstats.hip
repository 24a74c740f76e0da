// Validation statistics of the pre-training tasks (P/train_r2r_goat.py:438-583 validate_mlm / _mrc / _sap / _cfp,
// P/train_reverie_goat.py:587-612 validate_og): per-row loss and hit, and their sums, without a host read per batch.
//   goat_val_rows    hard:  loss[m] = logsumexp(row) - row[label]          hit[m] = (argmax(row) == label)
//                           (F.cross_entropy(reduction='sum') and `scores.max(dim=-1)[1] == labels`, row by row)
//                    soft:  loss[m] = sum_n xlogy(t, t) - t * log_softmax(row)[n]      hit[m] = (argmax(row) == argmax(t))
//                           (F.kl_div(log_softmax, t, reduction='sum') and compute_accuracy_for_soft_targets)
//   goat_val_cfp     the three symmetric InfoNCE problems of validate_cfp, one workgroup per (modality, sample)
//   goat_val_reduce  one workgroup: (sum of losses, hits, counted rows) ADDED into a float64 [3] slot
// Plain vector stores only.  No atomics and no waiting between workgroups: every sum has one writer and a fixed order, so two runs
// of the same call give the same bits.
//
// goat_val_rows reads every logit ONCE: a thread keeps (running maximum m, exponential sum s rescaled to m, lowest index of m, and
// the label's logit or the three target sums) while it walks its columns.  State rules:
//   * m starts at -inf and s at 0.  A value above m rescales s by exp(m - v) (exp(-inf) = 0 on the first one); a finite value at or below
//     m adds exp(v - m), where m is finite.  A -inf value changes nothing, so (-inf) - (-inf) is never formed: masked slots, in whole
//     leading or trailing stretches of a row, cost a compare.  A NaN fails both compares and poisons s.
//   * two states merge as (max, rescaled sum): a side whose maximum IS the common one keeps its sum as it is (that covers -inf with
//     -inf), the other side is rescaled by exp(its m - max), a finite or -inf exponent.  On equal maxima the lower index wins, so every
//     argmax is the lowest index among the maxima whatever the thread layout.
//   * a row of only -inf ends with s = 0: lse = -inf, loss = -inf - (-inf) = NaN as torch gives; its argmax is index 0 as torch's.
// A row pointer needs float alignment only: up to three leading columns are peeled to the next 16-byte boundary, the body is read as
// 16-byte pieces, the tail column by column (the soft form does so when both rows sit at the same offset from a boundary, and walks
// column by column otherwise).
#include "common.hpp"

#include <limits.h>
#include <math.h>

namespace {

constexpr int VR_THREADS = 256;
// Rows of up to VR_WAVE_MAX columns get one wave each, four rows per block: a lane of a wave reads 4 columns per trip, so 1024 columns
// are at most 4 trips per lane — what a thread of the 256-thread block spends on 4096 columns — and the row needs neither LDS nor a
// barrier.  Wider rows get a block each.  The figure is read off the loop shapes above; it is not a measured optimum.
constexpr int VR_WAVE_MAX = 1024;

struct RowState {
  float m, s;      // running maximum, sum of exp(v - m)
  int ai;          // lowest index of m (INT_MAX: nothing above -inf seen)
  float xl;        // hard: the label's logit (0 where the thread did not meet it)
  float tm;        // soft: running maximum of the targets, its lowest index, and the three sums
  int ti;
  float a, b, t;   // sum xlogy(t, t), sum t * x, sum t over the columns with t != 0
};

__device__ __forceinline__ void rs_init(RowState& r) {
  r.m = -INFINITY; r.s = 0.f; r.ai = INT_MAX; r.xl = 0.f;
  r.tm = -INFINITY; r.ti = INT_MAX; r.a = 0.f; r.b = 0.f; r.t = 0.f;
}

__device__ __forceinline__ void rs_logit(RowState& r, float v, int idx) {
  if (v > r.m) {
    r.s = r.s * __expf(r.m - v) + 1.f;
    r.m = v;
    r.ai = idx;
  } else if (v > -INFINITY) {
    r.s += __expf(v - r.m);
  } else if (v != v) {
    r.s = v;
  }
}

template <bool SOFT>
__device__ __forceinline__ void rs_step(RowState& r, float v, float t, int idx, int label) {
  rs_logit(r, v, idx);
  if (SOFT) {
    if (t > r.tm) { r.tm = t; r.ti = idx; }
    if (t != 0.f) {               // a zero target contributes 0 (xlogy(0, 0) = 0, and 0 * a masked -inf logit is not formed)
      r.a += t * __logf(t);
      r.b += t * v;
      r.t += t;
    }
  } else {
    if (idx == label) r.xl = v;
  }
}

// the columns of one row that thread `tid` of `nthr` owns, in ascending order
template <bool SOFT>
__device__ __forceinline__ void rs_walk(RowState& r, const float* row, const float* trow, int N, int label, int tid, int nthr) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
  const bool vec = !SOFT || (int)((reinterpret_cast<uintptr_t>(trow) >> 2) & 3) == mis;
  if (!vec) {
    for (int c = tid; c < N; c += nthr) rs_step<SOFT>(r, row[c], trow[c], c, label);
    return;
  }
  const int head = min((4 - mis) & 3, N);
  const int n4 = (N - head) >> 2;
  if (tid < head) rs_step<SOFT>(r, row[tid], SOFT ? trow[tid] : 0.f, tid, label);
  for (int q = tid; q < n4; q += nthr) {
    const int c = head + q * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (SOFT) t = *reinterpret_cast<const f32x4*>(trow + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) rs_step<SOFT>(r, v[e], t[e], c + e, label);
  }
  const int c = head + n4 * 4 + tid;
  if (c < N) rs_step<SOFT>(r, row[c], SOFT ? trow[c] : 0.f, c, label);      // (at most three tail columns; tid < 3 < nthr)
}

__device__ __forceinline__ void rs_merge(float& m, float& s, int& ai, float om, float os, int oi) {
  const float M = fmaxf(m, om);
  const float sa = (m == M) ? s : s * __expf(m - M);
  const float sb = (om == M) ? os : os * __expf(om - M);
  if (om > m || (om == m && oi < ai)) ai = oi;
  m = M;
  s = sa + sb;
}
__device__ __forceinline__ void rs_merge_arg(float& m, int& ai, float om, int oi) {
  if (om > m || (om == m && oi < ai)) { m = om; ai = oi; }
}

// butterfly over the wave: every lane ends with the row's state (a + b is commutative, so all lanes hold the same bits)
template <bool SOFT>
__device__ __forceinline__ void rs_wave(RowState& r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(r.m, o, 64), os = __shfl_xor(r.s, o, 64);
    const int oi = __shfl_xor(r.ai, o, 64);
    rs_merge(r.m, r.s, r.ai, om, os, oi);
    if (SOFT) {
      const float otm = __shfl_xor(r.tm, o, 64);
      const int oti = __shfl_xor(r.ti, o, 64);
      rs_merge_arg(r.tm, r.ti, otm, oti);
      r.a += __shfl_xor(r.a, o, 64);
      r.b += __shfl_xor(r.b, o, 64);
      r.t += __shfl_xor(r.t, o, 64);
    } else {
      r.xl += __shfl_xor(r.xl, o, 64);
    }
  }
}

template <bool SOFT>
__device__ __forceinline__ void rs_finish(const RowState& r, int N, int label, float* loss, int* hit) {
  const float lse = r.m + __logf(r.s);
  const int am = r.ai == INT_MAX ? 0 : r.ai;
  const bool poisoned = r.s != r.s;                      // a NaN logit: NaN loss, hit 0
  if (SOFT) {
    *loss = r.a - r.b + lse * r.t;
    *hit = (!poisoned && am == (r.ti == INT_MAX ? 0 : r.ti)) ? 1 : 0;
  } else {
    // a label past the row: NaN instead of a read out of bounds (the rule of ce_fwd_kernel); it can equal no argmax
    *loss = label < N ? lse - r.xl : __builtin_nanf("");
    *hit = (!poisoned && am == label) ? 1 : 0;
  }
}

struct ValRowsArgs {
  const float* logits;
  int64_t ld;
  int M, N;
  const int64_t* labels;
  const float* soft;
  int64_t ld_soft;
  float* row_loss;
  int32_t* row_hit;
};

// a negative label: an ignored row, loss 0 and hit 0, never read (goat_val_reduce leaves it out of the row count)
__device__ __forceinline__ bool vr_label(const ValRowsArgs& a, int m, int& label) {
  const int64_t l = a.labels[m];
  label = l > (int64_t)INT_MAX ? INT_MAX : (int)l;      // (INT_MAX >= N: the NaN rule)
  return l >= 0;
}

// one wave per row, four rows per block
template <bool SOFT>
__global__ __launch_bounds__(VR_THREADS) void val_rows_wave_kernel(ValRowsArgs a) {
  const int m = blockIdx.x * (VR_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= a.M) return;                                  // (wave-uniform; no barrier below)
  int label = 0;
  if (!SOFT && !vr_label(a, m, label)) {
    if (lane == 0) { a.row_loss[m] = 0.f; a.row_hit[m] = 0; }
    return;
  }
  RowState r;
  rs_init(r);
  rs_walk<SOFT>(r, a.logits + (int64_t)m * a.ld, SOFT ? a.soft + (int64_t)m * a.ld_soft : nullptr, a.N, label, lane, 64);
  rs_wave<SOFT>(r);
  if (lane == 0) rs_finish<SOFT>(r, a.N, label, a.row_loss + m, a.row_hit + m);
}

// one block per row; the four wave states meet in LDS and are merged in ascending wave order
template <bool SOFT>
__global__ __launch_bounds__(VR_THREADS) void val_rows_block_kernel(ValRowsArgs a) {
  __shared__ RowState part[VR_THREADS / 64];
  const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int label = 0;
  if (!SOFT && !vr_label(a, m, label)) {                 // (block-uniform)
    if (threadIdx.x == 0) { a.row_loss[m] = 0.f; a.row_hit[m] = 0; }
    return;
  }
  RowState r;
  rs_init(r);
  rs_walk<SOFT>(r, a.logits + (int64_t)m * a.ld, SOFT ? a.soft + (int64_t)m * a.ld_soft : nullptr, a.N, label, threadIdx.x, VR_THREADS);
  rs_wave<SOFT>(r);
  if (lane == 0) part[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    r = part[0];
    for (int w = 1; w < VR_THREADS / 64; ++w) {
      const RowState& o = part[w];
      rs_merge(r.m, r.s, r.ai, o.m, o.s, o.ai);
      if (SOFT) {
        rs_merge_arg(r.tm, r.ti, o.tm, o.ti);
        r.a += o.a; r.b += o.b; r.t += o.t;
      } else {
        r.xl += o.xl;
      }
    }
    rs_finish<SOFT>(r, a.N, label, a.row_loss + m, a.row_hit + m);
  }
}

// ------------------------------------------------------------------------------------------------ CFP
struct ValCfpArgs {
  const float* x[3];      // gmap, vp, fused: [B, H]
  const float* txt;       // [B, H]
  int B, H, vec;
  float inv_tau;
  float* row_loss;        // [3, B]
  int32_t* row_hit;       // [3, B]
};

__device__ __forceinline__ float vc_dot(const float* a, const float* b, int H, int lane, bool vec) {
  float s = 0.f;
  if (vec) {
    for (int k = lane * 4; k < H; k += 256) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a + k), y = *reinterpret_cast<const f32x4*>(b + k);
      s += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
    }
  } else {
    for (int k = lane; k < H; k += 64) s += a[k] * b[k];
  }
  return wave_sum(s);
}

// grid (B, 3): block (i, k) forms S1[j] = x_k[i] . txt[j] / tau and S2[j] = txt[i] . x_k[j] / tau in LDS (one wave per j, lanes over
// H), then wave 0 closes CE(S1, i) and the argmax of S1, wave 1 closes CE(S2, i).  The -inf guards of the row kernels are not needed:
// a dot product of finite vectors is finite.  A NaN score fails the compare of the maximum and poisons the exponential sum: NaN loss,
// hit 0.
__global__ __launch_bounds__(256) void val_cfp_kernel(ValCfpArgs p) {
  extern __shared__ float vc_sh[];      // [2, B] scores, then the two half losses
  float* half_loss = vc_sh + 2 * p.B;
  const int i = blockIdx.x, k = blockIdx.y, B = p.B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* xk = p.x[k];
  const float* xi = xk + (int64_t)i * p.H;
  const float* ti = p.txt + (int64_t)i * p.H;
  for (int j = wave; j < B; j += 4) {
    const float s1 = vc_dot(xi, p.txt + (int64_t)j * p.H, p.H, lane, p.vec);
    const float s2 = vc_dot(ti, xk + (int64_t)j * p.H, p.H, lane, p.vec);
    if (lane == 0) {
      vc_sh[j] = s1 * p.inv_tau;
      vc_sh[B + j] = s2 * p.inv_tau;
    }
  }
  __syncthreads();
  if (wave < 2) {
    const float* S = vc_sh + wave * B;
    float m = -INFINITY;
    int ai = INT_MAX;
    for (int j = lane; j < B; j += 64)
      if (S[j] > m) { m = S[j]; ai = j; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(ai, o, 64);
      rs_merge_arg(m, ai, om, oi);
    }
    float l = 0.f;
    for (int j = lane; j < B; j += 64) l += __expf(S[j] - m);
    l = wave_sum(l);
    if (lane == 0) {
      half_loss[wave] = m + __logf(l) - S[i];
      if (wave == 0) p.row_hit[(int64_t)k * B + i] = (l == l && ai == i) ? 1 : 0;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) p.row_loss[(int64_t)k * B + i] = 0.5f * (half_loss[0] + half_loss[1]);
}

// ------------------------------------------------------------------------------------------------ reduce
constexpr int RD_THREADS = 256;

// thread t sums rows t, t + 256, ... in ascending order (double), then a fixed binary tree over the 256 partials in LDS
__global__ __launch_bounds__(RD_THREADS) void val_reduce_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ row_hit,
                                                                const int64_t* __restrict__ labels, int M, double* acc) {
  __shared__ double sl[RD_THREADS];
  __shared__ int64_t sh[RD_THREADS], sr[RD_THREADS];
  const int t = threadIdx.x;
  double loss = 0.0;
  int64_t hits = 0, rows = 0;
  for (int m = t; m < M; m += RD_THREADS) {
    loss += (double)row_loss[m];
    hits += row_hit[m];
    rows += (labels == nullptr || labels[m] >= 0) ? 1 : 0;
  }
  sl[t] = loss; sh[t] = hits; sr[t] = rows;
  __syncthreads();
  for (int w = RD_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) {
      sl[t] += sl[t + w];
      sh[t] += sh[t + w];
      sr[t] += sr[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {                       // (launches on one stream run in order: the slot has one writer at a time)
    acc[0] += sl[0];
    acc[1] += (double)sh[0];
    acc[2] += (double)sr[0];
  }
}

}  // namespace

extern "C" int goat_val_rows(void* stream, const float* logits, int64_t ld, int M, int N, const int64_t* labels, const float* soft,
                             int64_t ld_soft, float* row_loss, int32_t* row_hit) {
  if (!logits || !row_loss || !row_hit || ((labels == nullptr) == (soft == nullptr))) return GOAT_E_ARG;
  if (M < 1 || N < 1 || ld < N || (soft && ld_soft < N)) return GOAT_E_SHAPE;
  ValRowsArgs a = {logits, ld, M, N, labels, soft, ld_soft, row_loss, row_hit};
  return bool_dispatch(soft != nullptr, [&](auto sf) -> int {
    constexpr bool SOFT = decltype(sf)::value;
    if (N <= VR_WAVE_MAX)
      hipLaunchKernelGGL(val_rows_wave_kernel<SOFT>, dim3((M + 3) / 4), dim3(VR_THREADS), 0, ST(stream), a);
    else
      hipLaunchKernelGGL(val_rows_block_kernel<SOFT>, dim3(M), dim3(VR_THREADS), 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_val_cfp(void* stream, const float* const* x, const float* txt, int B, int H, float temperature, float* row_loss,
                            int32_t* row_hit) {
  if (!x || !x[0] || !x[1] || !x[2] || !txt || !row_loss || !row_hit) return GOAT_E_ARG;
  if (B < 1 || B > GOAT_VAL_CFP_MAX_B || H < 1 || !(temperature > 0.f)) return GOAT_E_SHAPE;
  ValCfpArgs p;
  uintptr_t bits = reinterpret_cast<uintptr_t>(txt);
  for (int k = 0; k < 3; ++k) {
    p.x[k] = x[k];
    bits |= reinterpret_cast<uintptr_t>(x[k]);
  }
  p.txt = txt;
  p.B = B;
  p.H = H;
  p.vec = ((H & 3) == 0 && (bits & 15) == 0) ? 1 : 0;      // 16-byte pieces where every row starts on a boundary
  p.inv_tau = 1.f / temperature;
  p.row_loss = row_loss;
  p.row_hit = row_hit;
  hipLaunchKernelGGL(val_cfp_kernel, dim3(B, 3), dim3(256), (size_t)(2 * B + 2) * sizeof(float), ST(stream), p);
  GOAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int goat_val_reduce(void* stream, const float* row_loss, const int32_t* row_hit, const int64_t* labels, int M, double* acc) {
  if (!row_loss || !row_hit || !acc) return GOAT_E_ARG;
  if (M < 1) return GOAT_E_SHAPE;
  hipLaunchKernelGGL(val_reduce_kernel, dim3(1), dim3(RD_THREADS), 0, ST(stream), row_loss, row_hit, labels, M, acc);
  GOAT_LAUNCH_CHECK();
  return 0;
}
