// Beside the GEMMs of a Linear: column sums (bias gradient), transpose (+ column sums), weight gradient of a short-input Linear.
#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------ column sums
// block = 256 threads = 64 columns x 4 row lanes; each block walks a strip of rows, one atomic per column.
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int64_t ld, int R, int C,
                                                     float* __restrict__ colsum, int rows_per_block) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(R, r0 + rows_per_block);
  float acc = 0.f;
  if (c < C)
    for (int r = r0 + ty; r < r1; r += 4) acc += to_f(x[(int64_t)r * ld + c]);
  part[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && c < C) atomicAdd(colsum + c, part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx]);
}

// ------------------------------------------------------------------------------------ transpose
// 64x64 tiles through LDS; each block walks RT consecutive row tiles of one column tile so the column
// sums (bias gradient) cost one atomic per column per block.
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ in, int64_t ld_in, T* __restrict__ out,
                                                        int64_t ld_out, int R, int C, float* __restrict__ colsum, int RT) {
  __shared__ T tile[64][66];
  __shared__ float csum[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // ty 0..3
  const int c0 = blockIdx.y * 64;
  float acc = 0.f;
  for (int t = 0; t < RT; ++t) {
    const int r0 = (blockIdx.x * RT + t) * 64;
    if (r0 >= R && r0 >= (int)ld_out) break;
#pragma unroll 4
    for (int i = ty; i < 64; i += 4) {
      const int r = r0 + i, c = c0 + tx;
      T v = (T)0.f;
      if (r < R && c < C) v = in[(int64_t)r * ld_in + c];
      tile[i][tx] = v;
      acc += to_f(v);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = ty; i < 64; i += 4) {
      const int c = c0 + i, r = r0 + tx;
      if (c < C && r < (int)ld_out) out[(int64_t)c * ld_out + r] = tile[tx][i];
    }
    __syncthreads();
  }
  if (colsum) {
    csum[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && c0 + tx < C) atomicAdd(colsum + c0 + tx, csum[0][tx] + csum[1][tx] + csum[2][tx] + csum[3][tx]);
  }
}

// ------------------------------------------------------------------------------------ weight gradient of a short-input Linear
// dW[n, k] += sum_r dy[r, n] x[r, k] ; dbias[n] += sum_r dy[r, n]   for K <= 16 input features (the 7- / 14-wide position Linears,
// P/model/vilmodel_goat.py:300-303,406,475): block = 128 output columns x a chunk of rows, lane = 2 columns, wave = row phase.
// Replaces a padded-K GEMM into a temporary + slice copy + autograd's `grad += dW` (4 launches per Linear and step).
constexpr int SK_MAXK = 16, SK_BATCH = 8;
template <typename T, int KP, int SK_ROWS>      // SK_ROWS: rows per block (128; 32 for short inputs so that the grid still covers the chip)
__global__ __launch_bounds__(256) void wgrad_smallk_kernel(const T* __restrict__ dy, int64_t ld_dy, const T* __restrict__ x,
                                                           int64_t ld_x, int rows, int N, int K, float* __restrict__ dw,
                                                           int64_t ld_dw, float* __restrict__ dbias) {
  __shared__ float sm[4][128][SK_MAXK + 1];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (row indices stay scalar: x rows
  const int n0 = blockIdx.x * 128 + lane * 2;                                                    //  come through the scalar cache)
  const int r0 = blockIdx.y * SK_ROWS, r1 = min(rows, r0 + SK_ROWS);
  float acc[2][SK_MAXK], bsum[2] = {0.f, 0.f};
#pragma unroll
  for (int k = 0; k < SK_MAXK; ++k) { acc[0][k] = 0.f; acc[1][k] = 0.f; }
  const bool in0 = n0 < N, in1 = n0 + 1 < N;
  // SK_BATCH rows per trip: all their loads are issued before the first multiply (the kernel is latency-bound otherwise)
  for (int rb = r0 + wave * SK_BATCH; rb < r1; rb += 4 * SK_BATCH) {
    constexpr int EPC = DT<T>::EPC, NCH = KP / EPC;
    float d0[SK_BATCH], d1[SK_BATCH], xv[SK_BATCH][KP];
#pragma unroll
    for (int u = 0; u < SK_BATCH; ++u) {
      const int r = rb + u;
      const bool live = r < r1;
      d0[u] = (live && in0) ? to_f(dy[(int64_t)r * ld_dy + n0]) : 0.f;
      d1[u] = (live && in1) ? to_f(dy[(int64_t)r * ld_dy + n0 + 1]) : 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {          // one 16-byte load per chunk of the row (same address in every lane)
        Chunk<T> ch;
        if (live) ch.load(x + (int64_t)r * ld_x + c * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) xv[u][c * EPC + e] = live ? ch.v[e] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < SK_BATCH; ++u) {
      bsum[0] += d0[u]; bsum[1] += d1[u];
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        acc[0][k] += d0[u] * xv[u][k];
        acc[1][k] += d1[u] * xv[u][k];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
#pragma unroll
    for (int k = 0; k < SK_MAXK; ++k) sm[wave][lane * 2 + c][k] = acc[c][k];
    sm[wave][lane * 2 + c][SK_MAXK] = bsum[c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 128 * (K + 1); i += 256) {
    const int c = i / (K + 1), k = i % (K + 1), n = blockIdx.x * 128 + c;
    if (n >= N) continue;
    const int kk = k < K ? k : SK_MAXK;
    const float v = sm[0][c][kk] + sm[1][c][kk] + sm[2][c][kk] + sm[3][c][kk];
    if (k < K) atomicAdd(dw + (int64_t)n * ld_dw + k, v);
    else if (dbias) atomicAdd(dbias + n, v);
  }
}

}  // namespace

extern "C" int goat_colsum(void* stream, int dtype, const void* x, int64_t ld, int R, int C, float* colsum) {
  if (!x || !colsum) return GOAT_E_ARG;
  if (R <= 0 || C <= 0) return GOAT_E_SHAPE;
  const int cb = (C + 63) / 64;
  int rb = (1024 + cb - 1) / cb;
  if (rb > (R + 31) / 32) rb = (R + 31) / 32;
  if (rb < 1) rb = 1;
  const int rows_per_block = (R + rb - 1) / rb;
  dim3 grid(cb, (R + rows_per_block - 1) / rows_per_block);
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(256), 0, ST(stream), (const T*)x, ld, R, C, colsum, rows_per_block);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_transpose(void* stream, int dtype, const void* in, int64_t ld_in, void* out, int64_t ld_out, int R,
                              int C, float* colsum) {
  if (!in || !out) return GOAT_E_ARG;
  if (R <= 0 || C <= 0 || ld_out < R || ld_in < C) return GOAT_E_SHAPE;
  const int rtiles = (int)((ld_out + 63) / 64), ctiles = (C + 63) / 64;
  int RT = 1;
  while (RT < 16 && (int64_t)((rtiles + 2 * RT - 1) / (2 * RT)) * ctiles >= 1024) RT *= 2;
  dim3 grid((rtiles + RT - 1) / RT, ctiles);
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(transpose_kernel<T>, grid, dim3(256), 0, ST(stream), (const T*)in, ld_in, (T*)out, ld_out, R, C, colsum, RT);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_wgrad_smallk(void* stream, int dtype, const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int rows,
                                 int N, int K, float* dw, int64_t ld_dw, float* dbias) {
  if (!dy || !x || !dw) return GOAT_E_ARG;
  if (rows <= 0 || N <= 0 || K <= 0 || K > SK_MAXK) return GOAT_E_SHAPE;
  const int rc = rows >= 2048 ? 128 : 32;          // rows per block
  dim3 grid((N + 127) / 128, (rows + rc - 1) / rc);
  // x rows are read as whole 16-byte chunks (columns >= K are multiplied but never stored): rows padded and aligned to a chunk
  const int epc = dtype == GOAT_BF16 ? 8 : 4, kp = (K + epc - 1) / epc * epc;
  if (ld_x < kp || (ld_x % epc) || (reinterpret_cast<uintptr_t>(x) & 15)) return GOAT_E_SHAPE;
#define GOAT_SK_LAUNCH(T_, KP_)                                                                                              \
  do {                                                                                                                       \
    if (rc == 128)                                                                                                           \
      hipLaunchKernelGGL((wgrad_smallk_kernel<T_, KP_, 128>), grid, dim3(256), 0, ST(stream), (const T_*)dy, ld_dy, (const T_*)x, ld_x, \
                         rows, N, K, dw, ld_dw, dbias);                                                                      \
    else                                                                                                                     \
      hipLaunchKernelGGL((wgrad_smallk_kernel<T_, KP_, 32>), grid, dim3(256), 0, ST(stream), (const T_*)dy, ld_dy, (const T_*)x, ld_x, \
                         rows, N, K, dw, ld_dw, dbias);                                                                      \
  } while (0)
  if (dtype == GOAT_BF16) {
    if (kp == 8) GOAT_SK_LAUNCH(bf16_t, 8); else GOAT_SK_LAUNCH(bf16_t, 16);
  } else if (dtype == GOAT_F32) {
    if (kp == 4) GOAT_SK_LAUNCH(float, 4); else if (kp == 8) GOAT_SK_LAUNCH(float, 8);
    else if (kp == 12) GOAT_SK_LAUNCH(float, 12); else GOAT_SK_LAUNCH(float, 16);
  } else {
    return GOAT_E_ARG;
  }
#undef GOAT_SK_LAUNCH
  GOAT_LAUNCH_CHECK();
  return 0;
}
