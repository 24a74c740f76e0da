// goat_kmeans_{assign,csr,centres,pick}: Lloyd's k-means over the pooled front-door features and the draw of one member per cluster
// (the FACL dictionaries; M/utils/data.py:403-480 does this with sklearn and numpy on the host).  K <= 256 everywhere.
//
// goat_kmeans_assign — ONE wave per 32 rows, no LDS, no barrier.  The scores x_i·c_k are a [32 rows] x [32 centres] MFMA tile per
//   centre tile (exact float32: v_mfma_f32_32x32x2_f32 through mma32; bf16 rows are promoted, nothing is ever rounded to bf16), all
//   ceil(K/32) tiles of a row tile accumulate side by side so that X is read once.  The operand fragments a lane already holds give
//   the norms for free: a lane sees half of the k-range of row (lane&31) and of centre (lane&31), the other half sits in lane^32.
//   Epilogue: per accumulator slot r the lanes of a half-wave hold the scores of ONE row against 32 centres; a lane first folds its
//   tiles (ascending, strict <), then five (value, index) shuffles fold the half-wave, the lower index winning equal values.
//   Rows >= N and centres >= K are loaded from the last valid row / centre (never out of bounds) and masked afterwards.
// goat_kmeans_csr — ONE block of 1024 threads, thread = (row segment, cluster): count, exclusive scans in LDS, then the same walk
//   again placing the rows.  Every thread walks its rows in ascending order and the segments are ascending, so the sort is stable.
// goat_kmeans_centres — a block per (cluster, slab of 32 columns): 8 lanes cover the slab in 16-byte pieces (one 128-byte line of
//   a float32 row), 32 row groups stride the cluster's members; the groups are added through LDS in ascending order.  A cluster that
//   holds every row is therefore spread over D/32 workgroups x 32 row groups and the sum order depends on nothing but (order, start).
// goat_kmeans_pick — a block per cluster: thread 0 draws, everyone copies the row B times in 16-byte pieces.
#include <limits.h>
#include "common.hpp"

namespace {

constexpr int KM_MAXK = 256;

__device__ __forceinline__ f32x4 km_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 km_load4(const bf16_t* p) {
  const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
  f32x4 r = {(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
  return r;
}
__device__ __forceinline__ float km_sq(float acc, const f32x4& v) {
  return fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], fmaf(v[0], v[0], acc))));
}

struct AssignArgs {
  const void* X;
  int64_t ld;
  const float* C;
  int32_t* labels;
  float* mind2;
  int32_t* changed;
  int N, D, K;
};

template <typename T, int NT>
__global__ __launch_bounds__(64) void kmeans_assign_kernel(AssignArgs a) {
  const int lane = threadIdx.x, half = lane >> 5, l31 = lane & 31;
  const int row0 = blockIdx.x * 32;
  const int arow = min(row0 + l31, a.N - 1);
  const T* xp = reinterpret_cast<const T*>(a.X) + (int64_t)arow * a.ld + 4 * half;
  const float* cp[NT];
  f32x16 acc[NT];
  float cn[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    cp[t] = a.C + (int64_t)min(t * 32 + l31, a.K - 1) * a.D + 4 * half;
    cn[t] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  }
  float xn = 0.f;
  for (int k0 = 0; k0 < a.D; k0 += 8) {
    const f32x4 xa = km_load4(xp + k0);
    xn = km_sq(xn, xa);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x4 cb = km_load4(cp[t] + k0);
      cn[t] = km_sq(cn[t], cb);
      mma32(acc[t], xa, cb);
    }
  }
  xn += __shfl_xor(xn, 32, 64);                 // lane j and lane j + 32: ||x||² of row row0 + j
#pragma unroll
  for (int t = 0; t < NT; ++t) cn[t] += __shfl_xor(cn[t], 32, 64);

  float myb = INFINITY;
  int myi = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {                // slot r: row c_row(r, lane) against centre t * 32 + l31
    float best = INFINITY;
    int idx = l31;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = t * 32 + l31;
      float s = fmaf(-2.f, acc[t][r], cn[t]);
      if (col >= a.K || s != s) s = INFINITY;
      if (t == 0 || s < best) { best = s; idx = col; }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (ov < best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (l31 == r) { myb = best; myi = idx; }    // (centre 0 always competes, so idx < K even when every score is +inf)
  }
  const int lrow = c_row(l31 & 15, lane);       // lanes 0..15 of each half-wave write the 16 rows of that half
  const float xnr = __shfl(xn, lrow, 64);
  const int row = row0 + lrow;
  int diff = 0;
  if (l31 < 16 && row < a.N) {
    diff = a.labels[row] != myi;
    a.labels[row] = myi;
    if (a.mind2) a.mind2[row] = fmaxf(0.f, xnr + myb);
  }
  if (a.changed) {
    const unsigned long long m = __ballot(diff);
    if (lane == 0 && m) atomicAdd(a.changed, (int)__popcll(m));
  }
}

struct CsrArgs {
  const int32_t* labels;
  int32_t* start;
  int32_t* order;
  int N, K, lg;       // lg: log2 of K rounded up to a power of two
};

constexpr int CSR_THREADS = 1024;

__global__ __launch_bounds__(CSR_THREADS) void kmeans_csr_kernel(CsrArgs a) {
  __shared__ int cnt[CSR_THREADS];              // [segment][cluster]
  __shared__ int total[KM_MAXK];
  __shared__ int sstart[KM_MAXK + 1];
  const int tid = threadIdx.x, kpad = 1 << a.lg, k = tid & (kpad - 1), seg = tid >> a.lg, S = CSR_THREADS >> a.lg;
  const int64_t L = ((int64_t)a.N + S - 1) / S;
  const int i0 = (int)min((int64_t)seg * L, (int64_t)a.N), i1 = (int)min((int64_t)i0 + L, (int64_t)a.N);
  int c = 0;
  if (k < a.K)
    for (int i = i0; i < i1; ++i) c += a.labels[i] == k;
  cnt[tid] = c;
  __syncthreads();
  if (tid < kpad) {
    int run = 0;
    for (int s = 0; s < S; ++s) {
      const int v = cnt[s * kpad + tid];
      cnt[s * kpad + tid] = run;
      run += v;
    }
    total[tid] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int j = 0; j < a.K; ++j) {
      sstart[j] = run;
      run += total[j];
    }
    sstart[a.K] = run;
  }
  __syncthreads();
  if (tid <= a.K) a.start[tid] = sstart[tid];
  if (k < a.K) {
    int pos = sstart[k] + cnt[tid];
    for (int i = i0; i < i1; ++i)
      if (a.labels[i] == k) a.order[pos++] = i;
  }
}

struct CentreArgs {
  const void* X;
  int64_t ld;
  const int32_t* order;
  const int32_t* start;
  float* C;
  int N, D, K;
};

constexpr int CT_RG = 32, CT_CG = 8;            // row groups x 16-byte column pieces: a slab of 32 columns per block

template <typename T>
__global__ __launch_bounds__(CT_RG * CT_CG) void kmeans_centres_kernel(CentreArgs a) {
  __shared__ f32x4 red[CT_RG][CT_CG];
  const int k = blockIdx.x, cg = threadIdx.x % CT_CG, rg = threadIdx.x / CT_CG;
  const int col = (blockIdx.y * CT_CG + cg) * 4;
  const int s0 = a.start[k], s1 = a.start[k + 1];
  if (s0 < 0 || s1 > a.N || s1 <= s0) return;   // (block-uniform) empty cluster: its row of C stays as it is
  const T* X = reinterpret_cast<const T*>(a.X);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (col < a.D)
    for (int j = s0 + rg; j < s1; j += CT_RG) {
      const int row = a.order[j];
      if ((unsigned)row < (unsigned)a.N) acc += km_load4(X + (int64_t)row * a.ld + col);
    }
  red[rg][cg] = acc;
  __syncthreads();
  if (rg == 0 && col < a.D) {
    f32x4 s = red[0][cg];
#pragma unroll 8
    for (int g = 1; g < CT_RG; ++g) s += red[g][cg];
    const float n = (float)(s1 - s0);
    const f32x4 mean = {s[0] / n, s[1] / n, s[2] / n, s[3] / n};
    *reinterpret_cast<f32x4*>(a.C + (int64_t)k * a.D + col) = mean;
  }
}

struct PickArgs {
  const void* X;
  int64_t ld;
  const int32_t* order;
  const int32_t* start;
  void* out;
  int32_t* picked;
  int N, D, K, B;
  uint64_t seed, offset;
  const uint64_t* rng_dev;
};

template <typename T>
__global__ __launch_bounds__(256) void kmeans_pick_kernel(PickArgs a) {
  constexpr int NE = DT<T>::EPC;
  __shared__ int srow;
  const int k = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    const int s0 = a.start[k], s1 = a.start[k + 1];
    int row = -1;
    if (s0 >= 0 && s1 <= a.N && s1 > s0) {
      const GoatRng rng(a.seed + (a.rng_dev ? *a.rng_dev : 0ull));
      const uint32_t h = rng.pair_bits(a.offset + (uint64_t)k);
      row = a.order[s0 + (int)__umulhi(h, (uint32_t)(s1 - s0))];       // floor(u * n), u = h / 2^32
      if ((unsigned)row >= (unsigned)a.N) row = -1;
    }
    a.picked[k] = row;
    srow = row;
  }
  __syncthreads();
  const int row = srow;
  const int cpr = a.D / NE;
  const T* src = reinterpret_cast<const T*>(a.X) + (int64_t)max(row, 0) * a.ld;
  T* out = reinterpret_cast<T*>(a.out);
  for (int i = tid; i < a.B * cpr; i += 256) {
    const int b = i / cpr, c = i % cpr;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= 0) v = *reinterpret_cast<const f32x4*>(src + c * NE);
    *reinterpret_cast<f32x4*>(out + ((int64_t)b * a.K + k) * a.D + c * NE) = v;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the limits X shares between the entry points: 1 <= K <= 256, D a multiple of 8, dense 16-byte aligned rows
int check_x(int dtype, const void* X, int64_t ld, int N, int D, int K) {
  if (N < 1 || K < 1 || K > KM_MAXK || D < 8 || (D % 8) != 0 || ld < D) return GOAT_E_SHAPE;
  if ((ld % (dtype == GOAT_BF16 ? 8 : 4)) != 0 || !aligned16(X)) return GOAT_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int goat_kmeans_assign(void* stream, int dtype, const void* X, int64_t ld_x, const float* C, int32_t* labels, float* mind2,
                                  int32_t* changed, int N, int D, int K) {
  if (!X || !C || !labels) return GOAT_E_ARG;
  if (dtype != GOAT_F32 && dtype != GOAT_BF16) return GOAT_E_ARG;
  if (int e = check_x(dtype, X, ld_x, N, D, K)) return e;
  if (!aligned16(C)) return GOAT_E_SHAPE;
  AssignArgs a = {X, ld_x, C, labels, mind2, changed, N, D, K};
  const dim3 grid((N + 31) / 32), block(64);
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    if (K <= 32) hipLaunchKernelGGL((kmeans_assign_kernel<T, 1>), grid, block, 0, ST(stream), a);
    else if (K <= 64) hipLaunchKernelGGL((kmeans_assign_kernel<T, 2>), grid, block, 0, ST(stream), a);
    else if (K <= 128) hipLaunchKernelGGL((kmeans_assign_kernel<T, 4>), grid, block, 0, ST(stream), a);
    else hipLaunchKernelGGL((kmeans_assign_kernel<T, 8>), grid, block, 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_kmeans_csr(void* stream, const int32_t* labels, int32_t* start, int32_t* order, int N, int K) {
  if (!labels || !start || !order) return GOAT_E_ARG;
  if (N < 1 || K < 1 || K > KM_MAXK) return GOAT_E_SHAPE;
  int lg = 0;
  while ((1 << lg) < K) ++lg;
  CsrArgs a = {labels, start, order, N, K, lg};
  hipLaunchKernelGGL(kmeans_csr_kernel, dim3(1), dim3(CSR_THREADS), 0, ST(stream), a);
  GOAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int goat_kmeans_centres(void* stream, int dtype, const void* X, int64_t ld_x, const int32_t* order, const int32_t* start,
                                   float* C, int N, int D, int K) {
  if (!X || !order || !start || !C) return GOAT_E_ARG;
  if (dtype != GOAT_F32 && dtype != GOAT_BF16) return GOAT_E_ARG;
  if (int e = check_x(dtype, X, ld_x, N, D, K)) return e;
  if (!aligned16(C)) return GOAT_E_SHAPE;
  CentreArgs a = {X, ld_x, order, start, C, N, D, K};
  const dim3 grid(K, (D + 4 * CT_CG - 1) / (4 * CT_CG)), block(CT_RG * CT_CG);
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    hipLaunchKernelGGL(kmeans_centres_kernel<GOAT_DT_TYPE(dt)>, grid, block, 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_kmeans_pick(void* stream, int dtype, const void* X, int64_t ld_x, const int32_t* order, const int32_t* start,
                                void* out, int32_t* picked, int N, int D, int K, int B, uint64_t seed, uint64_t offset,
                                const uint64_t* rng_dev) {
  if (!X || !order || !start || !out || !picked) return GOAT_E_ARG;
  if (dtype != GOAT_F32 && dtype != GOAT_BF16) return GOAT_E_ARG;
  if (int e = check_x(dtype, X, ld_x, N, D, K)) return e;
  if (B < 1 || (int64_t)B * (D / 4) > INT_MAX || !aligned16(out)) return GOAT_E_SHAPE;
  PickArgs a = {X, ld_x, order, start, out, picked, N, D, K, B, seed, offset, rng_dev};
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    hipLaunchKernelGGL(kmeans_pick_kernel<GOAT_DT_TYPE(dt)>, dim3(K), dim3(256), 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}
