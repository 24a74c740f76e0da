// goat_dict_{accumulate,finish}: running per-slot means of picked feature rows — the BACL dictionaries (M/r2r/agent.py:713-848 appends
// one numpy row per picked token on the host and calls np.mean; M/do_utils/do_intervention.py:109-148 does the same per room type).
// The picked rows arrive one encoder batch at a time, so the state (sum, comp, count) lives in device memory between launches.
//
// goat_dict_accumulate — ONE wave per (slot, slab of 8 chunks of 16 bytes): lane = row lane (8) x chunk (8).  A slot's rows are taken
//   in pieces of DICT_PIECE = 64: row lane r adds rows r, r + 8, ... of the piece (8 at most, all loads issued before the adds), three
//   shuffles add the row lanes, and the piece sum is folded into the running pair with a two-sum step (Neumaier): comp collects what
//   the float32 add of sum lost.  No LDS, no barrier, no atomics: (slot, column) has one writer and the order of the additions is a
//   function of (rows, start) alone.  The wave of slab 0 also counts the rows it used.
// goat_dict_finish — a block per slot writes (sum + comp) / count to feats and to the B copies of out; a second, small launch forms
//   the total of the counts (every block for itself: K ints from the L2) and writes count / total, computed in float64.
#include "common.hpp"

namespace {

constexpr int DICT_PIECE = 64, DICT_RL = 8, DICT_CG = 8;      // rows per piece; row lanes x 16-byte chunks of a wave
constexpr int DICT_MAXK = 65535;

struct DictAccArgs {
  const void* X;
  int64_t ld, R;
  const int32_t* rows;
  const int32_t* start;
  float* sum;
  float* comp;
  int32_t* count;
  int P, D, K;
};

template <typename T>
__global__ __launch_bounds__(64) void dict_accumulate_kernel(DictAccArgs a) {
  constexpr int NE = DT<T>::EPC, PER = DICT_PIECE / DICT_RL;
  const int k = blockIdx.x, lane = threadIdx.x, cg = lane % DICT_CG, rl = lane / DICT_CG;
  const int col = (blockIdx.y * DICT_CG + cg) * NE;
  const int s0 = a.start[k], s1 = a.start[k + 1];
  if (s0 < 0 || s1 > a.P || s1 <= s0) return;      // (wave-uniform) no rows in this launch: pair and count stay as they are
  const bool live = col < a.D;
  const T* X = reinterpret_cast<const T*>(a.X);
  float s[NE], c[NE];
  if (rl == 0 && live) {
#pragma unroll
    for (int q = 0; q < NE; q += 4) {
      const f32x4 sv = *reinterpret_cast<const f32x4*>(a.sum + (int64_t)k * a.D + col + q);
      const f32x4 cv = *reinterpret_cast<const f32x4*>(a.comp + (int64_t)k * a.D + col + q);
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[q + e] = sv[e]; c[q + e] = cv[e]; }
    }
  }
  int used = 0;
  for (int p0 = s0; p0 < s1; p0 += DICT_PIECE) {
    Chunk<T> x[PER];
    bool ok[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int j = p0 + i * DICT_RL + rl;
      const int row = j < s1 ? a.rows[j] : -1;
      ok[i] = row >= 0 && (int64_t)row < a.R;
      if (ok[i] && live) x[i].load(X + (int64_t)row * a.ld + col);
    }
    float acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      used += ok[i];
      if (ok[i] && live) {
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] += x[i].v[e];
      }
    }
#pragma unroll
    for (int o = DICT_CG; o < 64; o <<= 1) {
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    }
    if (rl == 0 && live) {
#pragma unroll
      for (int e = 0; e < NE; ++e) {               // two-sum: t = fl(s + p), and what the add lost goes to c
        const float p = acc[e], t = s[e] + p;
        c[e] += fabsf(s[e]) >= fabsf(p) ? (s[e] - t) + p : (p - t) + s[e];
        s[e] = t;
      }
    }
  }
  if (rl == 0 && live) {
#pragma unroll
    for (int q = 0; q < NE; q += 4) {
      const f32x4 sv = {s[q], s[q + 1], s[q + 2], s[q + 3]}, cv = {c[q], c[q + 1], c[q + 2], c[q + 3]};
      *reinterpret_cast<f32x4*>(a.sum + (int64_t)k * a.D + col + q) = sv;
      *reinterpret_cast<f32x4*>(a.comp + (int64_t)k * a.D + col + q) = cv;
    }
  }
  if (blockIdx.y == 0) {                            // every chunk column saw the same rows: the lanes of chunk 0 hold the count
#pragma unroll
    for (int o = DICT_CG; o < 64; o <<= 1) used += __shfl_xor(used, o, 64);
    if (lane == 0 && used) a.count[k] += used;
  }
}

struct DictFinArgs {
  const float* sum;
  const float* comp;
  const int32_t* count;
  float* feats;
  void* out;
  void* out_pz;
  int B, D, K;
};

template <typename T>
__global__ __launch_bounds__(256) void dict_finish_feats_kernel(DictFinArgs a) {
  const int k = blockIdx.x;
  const int n = a.count[k];
  const float fn = (float)n;
  T* out = reinterpret_cast<T*>(a.out);
  for (int col = threadIdx.x * 4; col < a.D; col += 256 * 4) {
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
      const f32x4 sv = *reinterpret_cast<const f32x4*>(a.sum + (int64_t)k * a.D + col);
      const f32x4 cv = *reinterpret_cast<const f32x4*>(a.comp + (int64_t)k * a.D + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = (sv[e] + cv[e]) / fn;
    }
    if (a.feats) *reinterpret_cast<f32x4*>(a.feats + (int64_t)k * a.D + col) = m;
    if (out) {
      for (int b = 0; b < a.B; ++b) {
        T* dst = out + ((int64_t)b * a.K + k) * a.D + col;
        if constexpr (sizeof(T) == 4) {
          *reinterpret_cast<f32x4*>(dst) = m;
        } else {
          const bf16x4 v = {(bf16_t)m[0], (bf16_t)m[1], (bf16_t)m[2], (bf16_t)m[3]};
          *reinterpret_cast<bf16x4*>(dst) = v;
        }
      }
    }
  }
}

constexpr int PZ_THREADS = 256, PZ_MAXBLOCKS = 64;

template <typename T>
__global__ __launch_bounds__(PZ_THREADS) void dict_finish_pz_kernel(DictFinArgs a) {
  __shared__ long long part[PZ_THREADS];
  long long t = 0;
  for (int k = threadIdx.x; k < a.K; k += PZ_THREADS) t += max(a.count[k], 0);
  part[threadIdx.x] = t;
  __syncthreads();
  for (int o = PZ_THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  const double total = (double)part[0];
  T* pz = reinterpret_cast<T*>(a.out_pz);
  const int64_t n = (int64_t)a.B * a.K;
  for (int64_t i = (int64_t)blockIdx.x * PZ_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PZ_THREADS) {
    const int cnt = a.count[i % a.K];
    const float v = cnt > 0 ? (float)((double)cnt / total) : 0.f;       // float64 quotient, one rounding to float32
    pz[i] = from_f<T>(v);
  }
}

bool dict_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int goat_dict_accumulate(void* stream, int dtype, const void* X, int64_t ld_x, int64_t R, const int32_t* rows,
                                    const int32_t* start, float* sum, float* comp, int32_t* count, int P, int D, int K) {
  if (!X || !rows || !start || !sum || !comp || !count) return GOAT_E_ARG;
  if (dtype != GOAT_F32 && dtype != GOAT_BF16) return GOAT_E_ARG;
  if (K < 1 || K > DICT_MAXK || P < 1 || R < 1 || D < 8 || (D % 8) != 0 || ld_x < D) return GOAT_E_SHAPE;
  if ((ld_x % (dtype == GOAT_BF16 ? 8 : 4)) != 0 || !dict_aligned16(X) || !dict_aligned16(sum) || !dict_aligned16(comp)) return GOAT_E_SHAPE;
  DictAccArgs a = {X, ld_x, R, rows, start, sum, comp, count, P, D, K};
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    const int slab = DICT_CG * DT<T>::EPC;
    hipLaunchKernelGGL(dict_accumulate_kernel<T>, dim3(K, (D + slab - 1) / slab), dim3(64), 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_dict_finish(void* stream, int out_dtype, const float* sum, const float* comp, const int32_t* count, float* feats,
                                void* out, void* out_pz, int B, int D, int K) {
  if (!sum || !comp || !count) return GOAT_E_ARG;
  if (out_dtype != GOAT_F32 && out_dtype != GOAT_BF16) return GOAT_E_ARG;
  if (K < 1 || K > DICT_MAXK || B < 1 || D < 8 || (D % 8) != 0) return GOAT_E_SHAPE;
  if (!dict_aligned16(sum) || !dict_aligned16(comp) || !dict_aligned16(feats) || !dict_aligned16(out)) return GOAT_E_SHAPE;
  if (!feats && !out && !out_pz) return 0;
  DictFinArgs a = {sum, comp, count, feats, out, out_pz, B, D, K};
  return dtype_dispatch(out_dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    if (feats || out) {
      hipLaunchKernelGGL(dict_finish_feats_kernel<T>, dim3(K), dim3(256), 0, ST(stream), a);
      GOAT_LAUNCH_CHECK();
    }
    if (out_pz) {
      const int64_t n = (int64_t)B * K;
      const int blocks = (int)((n + PZ_THREADS - 1) / PZ_THREADS < PZ_MAXBLOCKS ? (n + PZ_THREADS - 1) / PZ_THREADS : PZ_MAXBLOCKS);
      hipLaunchKernelGGL(dict_finish_pz_kernel<T>, dim3(blocks), dim3(PZ_THREADS), 0, ST(stream), a);
      GOAT_LAUNCH_CHECK();
    }
    return 0;
  });
}
