// Residual + dropout + LayerNorm, forward and backward: one wave64 per row, 16-byte vector loads, wavefront shuffles for the
// reductions, statistics in f32.
#include <cstdlib>
#include "common.hpp"
#include <algorithm>
#include <vector>

namespace {

#ifndef GOAT_LN_ABL
#define GOAT_LN_ABL 0      // (ablation builds of scripts/ln_bench.py: 1 no column reduction, 2 no dropout hash, 4 no stores)
#endif
constexpr int MAXC_MAX = 8;  // 16-B chunks per lane kept in registers: H <= 64*MAXC*EPC (MAXC is a template parameter)
#define GOAT_LN_BWD_PARTS 512
#ifndef GOAT_LN_BWD_WAVES
// waves per block of the LayerNorm backward.  Isolated (scripts/ln_bench.py, atomic mode, 3840 rows): 4 -> 20.4 us, 8 -> 15.8, 16 -> 42.  Inside
// the step the kernel runs with deferred column partials (no atomics) and usually NEXT TO a GEMM of the other graph branch whose
// workgroups hold 96-112 KiB of a CU's 160 KiB LDS: an 8-wave block needs 48 KiB for its column reduction and fits beside such a
// workgroup only just or not at all, a 4-wave block (24 KiB) always does.  Same-box A/B of the whole step, three alternations (round 4):
// 8 waves 5.647 / 5.672 / 5.662 ms, 4 waves 5.579 / 5.598 / 5.614 ms; 2 waves (12 KiB, twice the partial rows) is slower again (+0.06 ms).
#define GOAT_LN_BWD_WAVES 4
#endif
#ifndef GOAT_LN_BWD768
#define GOAT_LN_BWD768 1     // bf16 rows of 768: ln_bwd768_kernel (0: the generic kernel; also GOAT_LN_BWD_GENERIC=1 in the environment)
#endif
#ifndef GOAT_LN_RIF
#define GOAT_LN_RIF 2      // rows in flight per wave (bf16); measured: 4 rows / fewer partial blocks are slower (8.52-8.80 vs 8.45 ms/step)
#endif

// ------------------------------------------------------------------------------------ LayerNorm fwd
template <typename T, int MAXC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float eps, float p, uint64_t seed, uint64_t offset,
                                                     const uint64_t* __restrict__ rng_dev, T* __restrict__ y, T* __restrict__ zout, float* __restrict__ mean,
                                                     float* __restrict__ rstd, int M, int H, float p_out, uint64_t offset_out,
                                                     const T* __restrict__ post_add) {
  constexpr int EPC = DT<T>::EPC;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  if (rng_dev) seed += *rng_dev;
  const GoatRng rng(seed);
  const int nchunk = H / EPC;
  const bool drop = p > 0.f;
  const uint32_t thr = goat_thr16(p);
  const float ks = drop ? 1.f / (1.f - p) : 1.f;
  Chunk<T> v[MAXC];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
      const int64_t base = (int64_t)row * H + c * EPC;
      v[i].load(x + base);
      if (drop) {
        const uint32_t km = rng.keep_bits<EPC>(offset + base, thr);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[i].v[e] = ((km >> e) & 1u) ? v[i].v[e] * ks : 0.f;
      }
      if (res) v[i].add(res + base);
      // round z to the storage type so forward statistics and backward recomputation agree
#pragma unroll
      for (int e = 0; e < EPC; ++e) v[i].v[e] = to_f(from_f<T>(v[i].v[e]));
      if (zout) v[i].store_stream(zout + base);
#pragma unroll
      for (int e = 0; e < EPC; ++e) sum += v[i].v[e];
    }
  }
  const float mu = wave_sum(sum) / H;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) { float d = v[i].v[e] - mu; var += d * d; }
    }
  }
  const float rs = rsqrtf(wave_sum(var) / H + eps);
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
      Chunk<T> o;
#pragma unroll
      for (int e = 0; e < EPC; ++e) o.v[e] = (v[i].v[e] - mu) * rs * gamma[c * EPC + e] + beta[c * EPC + e];
      // a second summand behind the norm: y = dropout(LayerNorm(z) + post_add) — the image embedding block adds the normalised
      // location features to the normalised view features (P/model/vilmodel_goat.py:340-344)
      if (post_add) o.add(post_add + (int64_t)row * H + c * EPC);
      if (p_out > 0.f) {       // dropout on the OUTPUT (embeddings: dropout(LayerNorm(e)), P/model/Bert_backbone.py:108-110)
        const uint32_t km = rng.keep_bits<EPC>(offset_out + (int64_t)row * H + c * EPC, goat_thr16(p_out));
        const float ko = 1.f / (1.f - p_out);
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.v[e] = ((km >> e) & 1u) ? o.v[e] * ko : 0.f;
      }
      o.store_stream(y + (int64_t)row * H + c * EPC);
    }
  }
}

// ------------------------------------------------------------------------------------ LayerNorm bwd
// grid = NPART blocks of 4 waves; wave w of block b walks rows (b*4+w), +4*NPART, ...
// partial dgamma/dbeta per block -> ws[block][2][H]; ln_bwd_reduce sums them.
template <typename T, int MAXC, int RIF, int NWV>
__global__ __launch_bounds__(64 * NWV) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dy2, const T* __restrict__ z,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, float p, uint64_t seed,
                                                     uint64_t offset, const uint64_t* __restrict__ rng_dev,
                                                     T* __restrict__ dx, T* __restrict__ dres,
                                                     float* __restrict__ ws, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                     const T* __restrict__ dx_add, int pre_add, int M, int H, float p_out,
                                                     uint64_t offset_out, T* __restrict__ d_post) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float lsum[];  // [NWV][2][H]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (rng_dev) seed += *rng_dev;
  const GoatRng rng(seed);
  const int nchunk = H / EPC;
  const bool drop = p > 0.f;
  const uint32_t thr = goat_thr16(p);
  const float ks = drop ? 1.f / (1.f - p) : 1.f;
  float dg[MAXC][EPC], db[MAXC][EPC], g[MAXC][EPC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      dg[i][e] = 0.f; db[i][e] = 0.f;
      const int c = lane + 64 * i;
      g[i][e] = (c < nchunk) ? gamma[c * EPC + e] : 0.f;
    }
  // RIF rows per wave in flight: the loads of both rows are issued before the first reduction (this kernel is
  // latency-bound on its 16-B loads, not on the shuffles)
  const int rstride = gridDim.x * NWV;
  for (int row0 = blockIdx.x * NWV + wave; row0 < M; row0 += RIF * rstride) {
    Chunk<T> vdy[RIF][MAXC], vz[RIF][MAXC];
    float mu[RIF], rs[RIF], c1[RIF], c2[RIF];
#pragma unroll
    for (int u = 0; u < RIF; ++u) { c1[u] = 0.f; c2[u] = 0.f; }
    bool live[RIF];
#pragma unroll
    for (int u = 0; u < RIF; ++u) {
      const int row = row0 + u * rstride;
      live[u] = row < M;
      mu[u] = live[u] ? mean[row] : 0.f;
      rs[u] = live[u] ? rstd[row] : 0.f;
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = lane + 64 * i;
        if (live[u] && c < nchunk) {
          const int64_t base = (int64_t)row * H + c * EPC;
          vdy[u][i].load(dy + base);
          vz[u][i].load(z + base);
          if (dy2) vdy[u][i].add(dy2 + base);   // second upstream gradient of the same tensor (its other consumer): summed here instead of by an add kernel
          if (p_out > 0.f) {     // forward dropped its OUTPUT with this mask: the gradient of the normalised value is masked the same way
            const uint32_t km = rng.keep_bits<EPC>(offset_out + base, goat_thr16(p_out));
            const float ko = 1.f / (1.f - p_out);
#pragma unroll
            for (int e = 0; e < EPC; ++e) vdy[u][i].v[e] = ((km >> e) & 1u) ? vdy[u][i].v[e] * ko : 0.f;
          }
          if (d_post) vdy[u][i].store_stream(d_post + base);      // gradient of the summand added behind the norm (post_add)
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RIF; ++u) {
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = lane + 64 * i;
        if (live[u] && c < nchunk) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) {
            const float xh = (vz[u][i].v[e] - mu[u]) * rs[u];
            const float d = vdy[u][i].v[e];
            dg[i][e] += d * xh;
            db[i][e] += d;
            const float dxh = d * g[i][e];
            c1[u] += dxh;
            c2[u] += dxh * xh;
            vz[u][i].v[e] = xh;
            vdy[u][i].v[e] = dxh;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RIF; ++u) {
      c1[u] = wave_sum(c1[u]) / H;
      c2[u] = wave_sum(c2[u]) / H;
    }
#pragma unroll
    for (int u = 0; u < RIF; ++u) {
      const int row = row0 + u * rstride;
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = lane + 64 * i;
        if (live[u] && c < nchunk) {
          const int64_t base = (int64_t)row * H + c * EPC;
          Chunk<T> o;
#pragma unroll
          for (int e = 0; e < EPC; ++e) o.v[e] = (vdy[u][i].v[e] - c1[u] - vz[u][i].v[e] * c2[u]) * rs[u];
#if GOAT_LN_ABL & 4
          asm volatile("" ::"v"(o.v[0]), "v"(o.v[EPC - 1]));
          continue;
#endif
          // gradient arriving at the PRE-NORM SUM z = residual + dropout(x) through its other consumer (the skip connection that
          // continues behind this LayerNorm): joins before the residual / dropout split
          if (dx_add && pre_add) o.add(dx_add + base);
          if (dres) o.store_stream(dres + base);
#if GOAT_LN_ABL & 2
          if (false) {
#else
          if (drop) {
#endif
            const uint32_t km = rng.keep_bits<EPC>(offset + base, thr);
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.v[e] = ((km >> e) & 1u) ? o.v[e] * ks : 0.f;
          }
          if (dx_add && !pre_add) o.add(dx_add + base);     // gradient of x arriving through its OTHER consumer (the skip connection of a pre-LN block): summed on store
          if (dx) o.store_stream(dx + base);
        }
      }
    }
  }
  // block reduction of the column partials
#if GOAT_LN_ABL & 1
#pragma unroll
  for (int i = 0; i < MAXC; ++i) asm volatile("" ::"v"(dg[i][0]), "v"(db[i][0]), "v"(dg[i][EPC - 1]), "v"(db[i][EPC - 1]));
  return;
#endif
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        lsum[(wave * 2 + 0) * H + c * EPC + e] = dg[i][e];
        lsum[(wave * 2 + 1) * H + c * EPC + e] = db[i][e];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * H; i += 64 * NWV) {
    const int which = i / H, col = i % H;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) s += lsum[(w * 2 + which) * H + col];
    if (ws != nullptr) ws[(int64_t)blockIdx.x * 2 * H + i] = s;          // deterministic mode: per-block partials + ln_bwd_reduce_kernel
    else atomicAdd((which == 0 ? dgamma : dbeta) + col, s);                // default: one float atomic per block and column into the
  }                                                                        // (pre-zeroed) gradient; no second launch
}

// ---- bf16, H = 768 (every LayerNorm of the model at its hidden size): the backward on a register diet.
// The generic kernel above keeps two rows in flight as float (16-byte chunks: the second chunk of a 768-wide row occupies half the
// lanes) and needs 192 VGPRs — two waves per SIMD, and ONE slot beside a 240-VGPR GEMM workgroup of the other graph branch (measured
// in the step: 18.9 us against 10.7 alone).  Here a lane owns 12 elements of a row as THREE 8-BYTE chunks (all 64 lanes busy), the
// row being reduced lives in float, the NEXT row of the wave is in flight in its packed bf16 form (12 registers for dy | z, converted
// on use): <= 96 VGPRs -> five waves per SIMD alone, two beside a GEMM wave.  Same arithmetic, order and results as ln_bwd_kernel.
__device__ __forceinline__ void goat_store_stream8(bf16_t* p, const bf16x4& v) {
#if GOAT_ROW_NT
  __builtin_nontemporal_store(v, reinterpret_cast<bf16x4*>(p));
#else
  *reinterpret_cast<bf16x4*>(p) = v;
#endif
}

template <int NWV, int RIF, bool DROP, bool DY2, bool EXTRA>
__device__ __forceinline__ void ln_bwd768_body(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ dy2,
                                                             const bf16_t* __restrict__ z, const float* __restrict__ gamma,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, float p,
                                                             uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_dev,
                                                             bf16_t* __restrict__ dx, bf16_t* __restrict__ dres, float* __restrict__ ws,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             const bf16_t* __restrict__ dx_add, int pre_add, int M, float p_out,
                                                             uint64_t offset_out, bf16_t* __restrict__ d_post) {
  constexpr int H = 768, NC = 3, E = 4;
  extern __shared__ float lsum[];  // [NWV][2][H] column partials, then gamma [H] (read per row: 12 registers less than holding it)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* __restrict__ lgam = lsum + NWV * 2 * H;
  float dg[NC][E], db[NC][E];
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i)
      *reinterpret_cast<f32x4*>(lgam + (lane + 64 * i) * E) = *reinterpret_cast<const f32x4*>(gamma + (lane + 64 * i) * E);
  }
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int e = 0; e < E; ++e) { dg[i][e] = 0.f; db[i][e] = 0.f; }
  __syncthreads();
  if (rng_dev) seed += *rng_dev;
  const int rstride = gridDim.x * NWV;
  for (int row0 = blockIdx.x * NWV + wave; row0 < M; row0 += RIF * rstride) {
    // RIF rows of the wave in flight in their packed form (the loads of all of them are issued before the first reduction)
    bf16x4 pdy[RIF][NC], pz[RIF][NC], pdy2[RIF][NC];
    float mus[RIF], rss[RIF];
#pragma unroll
    for (int u = 0; u < RIF; ++u) {
      const int row = row0 + u * rstride;
      if (row < M) {
        const uint32_t rb = (uint32_t)row * H + lane * E;      // (the launcher sends rows beyond 2^31 bytes to the generic kernel)
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          pdy[u][i] = *reinterpret_cast<const bf16x4*>(dy + rb + 64 * E * i);
          pz[u][i] = *reinterpret_cast<const bf16x4*>(z + rb + 64 * E * i);
          if (DY2) pdy2[u][i] = *reinterpret_cast<const bf16x4*>(dy2 + rb + 64 * E * i);
        }
        mus[u] = mean[row];
        rss[u] = rstd[row];
      }
    }
#pragma unroll
    for (int u = 0; u < RIF; ++u) {
      __builtin_amdgcn_sched_barrier(0);      // one row in float at a time: the conversions of row u + 1 stay behind row u's stores
      const int row = row0 + u * rstride;
      if (row >= M) break;
      float d[NC][E], xh[NC][E];
      const float mu = mus[u], rs = rss[u];
#pragma unroll
      for (int i = 0; i < NC; ++i)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          d[i][e] = (float)pdy[u][i][e];
          if (DY2) d[i][e] += (float)pdy2[u][i][e];      // the second upstream gradient of the same tensor (its other consumer)
          xh[i][e] = ((float)pz[u][i][e] - mu) * rs;
        }
      const uint32_t rbase = (uint32_t)row * H + lane * E;
      if (EXTRA) {
        if (p_out > 0.f) {       // forward dropped its OUTPUT with this mask
          const GoatRng rng(seed);
          const float ko = 1.f / (1.f - p_out);
#pragma unroll
          for (int i = 0; i < NC; ++i) {
            const uint32_t km = rng.keep_bits<E>(offset_out + rbase + 64 * E * i, goat_thr16(p_out));
#pragma unroll
            for (int e = 0; e < E; ++e) d[i][e] = ((km >> e) & 1u) ? d[i][e] * ko : 0.f;
          }
        }
        if (d_post) {
#pragma unroll
          for (int i = 0; i < NC; ++i) {
            bf16x4 t;
#pragma unroll
            for (int e = 0; e < E; ++e) t[e] = (bf16_t)d[i][e];
            goat_store_stream8(d_post + rbase + 64 * E * i, t);
          }
        }
      }
      float c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(lgam + (lane + 64 * i) * E);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float dd = d[i][e];
          dg[i][e] += dd * xh[i][e];
          db[i][e] += dd;
          const float dxh = dd * g[e];
          c1 += dxh;
          c2 += dxh * xh[i][e];
          d[i][e] = dxh;
        }
      }
      c1 = wave_sum(c1) / H;
      c2 = wave_sum(c2) / H;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const uint32_t base = rbase + 64 * E * i;
        float o[E];
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = (d[i][e] - c1 - xh[i][e] * c2) * rs;
        if (EXTRA && dx_add && pre_add) {
          const bf16x4 t = *reinterpret_cast<const bf16x4*>(dx_add + base);
#pragma unroll
          for (int e = 0; e < E; ++e) o[e] += (float)t[e];
        }
        if (dres) {
          bf16x4 t;
#pragma unroll
          for (int e = 0; e < E; ++e) t[e] = (bf16_t)o[e];
          goat_store_stream8(dres + base, t);
        }
        if (DROP) {
          const GoatRng rng(seed);
          const float ks = 1.f / (1.f - p);
          const uint32_t km = rng.keep_bits<E>(offset + base, goat_thr16(p));
#pragma unroll
          for (int e = 0; e < E; ++e) o[e] = ((km >> e) & 1u) ? o[e] * ks : 0.f;
        }
        if (EXTRA && dx_add && !pre_add) {
          const bf16x4 t = *reinterpret_cast<const bf16x4*>(dx_add + base);
#pragma unroll
          for (int e = 0; e < E; ++e) o[e] += (float)t[e];
        }
        if (dx) {
          bf16x4 t;
#pragma unroll
          for (int e = 0; e < E; ++e) t[e] = (bf16_t)o[e];
          goat_store_stream8(dx + base, t);
        }
      }
    }
  }
  // block reduction of the column partials (as ln_bwd_kernel)
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int col = (lane + 64 * i) * E;
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < E; ++e) { a[e] = dg[i][e]; b[e] = db[i][e]; }
    *reinterpret_cast<f32x4*>(&lsum[(wave * 2 + 0) * H + col]) = a;
    *reinterpret_cast<f32x4*>(&lsum[(wave * 2 + 1) * H + col]) = b;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * H; i += 64 * NWV) {
    const int which = i / H, col = i % H;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) s += lsum[(w * 2 + which) * H + col];
    if (ws != nullptr) ws[(int64_t)blockIdx.x * 2 * H + i] = s;
    else atomicAdd((which == 0 ? dgamma : dbeta) + col, s);
  }
}

#define GOAT_LN768_PARAMS                                                                                                         \
  const bf16_t *__restrict__ dy, const bf16_t *__restrict__ dy2, const bf16_t *__restrict__ z, const float *__restrict__ gamma,    \
      const float *__restrict__ mean, const float *__restrict__ rstd, float p, uint64_t seed, uint64_t offset,                      \
      const uint64_t *__restrict__ rng_dev, bf16_t *__restrict__ dx, bf16_t *__restrict__ dres, float *__restrict__ ws,              \
      float *__restrict__ dgamma, float *__restrict__ dbeta, const bf16_t *__restrict__ dx_add, int pre_add, int M, float p_out,     \
      uint64_t offset_out, bf16_t *__restrict__ d_post
#define GOAT_LN768_ARGS dy, dy2, z, gamma, mean, rstd, p, seed, offset, rng_dev, dx, dres, ws, dgamma, dbeta, dx_add, pre_add, M, p_out, offset_out, d_post
// the common forms (post-LN blocks: dropout, forked output) are held to 128 VGPRs = four waves per SIMD; the forms with a joining
// skip gradient / output dropout / post-add gradient (pre-LN panorama blocks, embeddings) would spill there: three waves per SIMD
template <int NWV, int RIF, bool DROP, bool DY2>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(4, 8))) void ln_bwd768_kernel(GOAT_LN768_PARAMS) {
  ln_bwd768_body<NWV, RIF, DROP, DY2, false>(GOAT_LN768_ARGS);
}
template <int NWV, int RIF, bool DROP, bool DY2>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(3, 8))) void ln_bwd768x_kernel(GOAT_LN768_PARAMS) {
  ln_bwd768_body<NWV, RIF, DROP, DY2, true>(GOAT_LN768_ARGS);
}

// 256 threads = 16 columns x 16 part-groups; every thread sums nparts/16 partials with 4 independent chains
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int nparts, int H, int accumulate) {
  __shared__ float red[16][17];
  const int cx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + cx;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < 2 * H) {
    int b = g;
    for (; b + 48 < nparts; b += 64) {
      s0 += ws[(int64_t)b * 2 * H + i];
      s1 += ws[(int64_t)(b + 16) * 2 * H + i];
      s2 += ws[(int64_t)(b + 32) * 2 * H + i];
      s3 += ws[(int64_t)(b + 48) * 2 * H + i];
    }
    for (; b < nparts; b += 16) s0 += ws[(int64_t)b * 2 * H + i];
  }
  red[g][cx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && i < 2 * H) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cx];
    float* dst = (i < H) ? dgamma + i : dbeta + (i - H);
    *dst = accumulate ? *dst + t : t;
  }
}

// Deferred reduction (goat_ln_bwd with accumulate == 2 leaves per-block partials behind): ONE launch at the end of the backward pass
// sums the partials of up to 64 LayerNorm calls into their (pre-zeroed / accumulating) gradient vectors.  blockIdx.y = entry.
struct LnPartial { const float* ws; float* dgamma; float* dbeta; int nparts; int pad; };
struct LnReduceArgs { LnPartial e[64]; int n; int H; };
__global__ __launch_bounds__(256) void ln_reduce_batched_kernel(LnReduceArgs a) {
  // entries are sorted by destination: the first entry of a run of equal destinations (a LayerNorm applied several times in one
  // backward pass: shared modules, BPTT) sums the whole run, the others leave — one writer per gradient word, fixed order
  __shared__ float red[16][17];
  const int e0 = blockIdx.y;
  if (e0 > 0 && a.e[e0 - 1].dgamma == a.e[e0].dgamma) return;
  const int H = a.H;
  const int cx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + cx;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int e = e0; e < a.n && a.e[e].dgamma == a.e[e0].dgamma; ++e) {
    const float* __restrict__ ws = a.e[e].ws;
    const int nparts = a.e[e].nparts;
    if (i < 2 * H) {
      int b = g;
      for (; b + 48 < nparts; b += 64) {
        s0 += ws[(int64_t)b * 2 * H + i];
        s1 += ws[(int64_t)(b + 16) * 2 * H + i];
        s2 += ws[(int64_t)(b + 32) * 2 * H + i];
        s3 += ws[(int64_t)(b + 48) * 2 * H + i];
      }
      for (; b < nparts; b += 16) s0 += ws[(int64_t)b * 2 * H + i];
    }
  }
  red[g][cx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && i < 2 * H) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cx];
    float* dst = (i < H) ? a.e[e0].dgamma + i : a.e[e0].dbeta + (i - H);
    *dst += t;
  }
}

__global__ __launch_bounds__(256) void zero2_kernel(float* __restrict__ a, float* __restrict__ b, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) { a[i] = 0.f; b[i] = 0.f; }
}

// ------------------------------------------------------------------------------------ launchers
template <typename T>
int ln_check(int H) {
  const int epc = DT<T>::EPC;
  if (H % epc) return GOAT_E_SHAPE;
  if (H > 64 * MAXC_MAX * epc) return GOAT_E_SHAPE;
  return 0;
}
template <typename T>
int ln_maxc(int H) {  // smallest instantiated chunk count covering H
  const int need = (H / DT<T>::EPC + 63) / 64;
  return need <= 1 ? 1 : need <= 2 ? 2 : need <= 3 ? 3 : need <= 4 ? 4 : 8;
}
#define GOAT_LN_DISPATCH(T_, H_, ...)                        \
  switch (ln_maxc<T_>(H_)) {                                 \
    case 1: { constexpr int MC = 1; __VA_ARGS__; } break;    \
    case 2: { constexpr int MC = 2; __VA_ARGS__; } break;    \
    case 3: { constexpr int MC = 3; __VA_ARGS__; } break;    \
    case 4: { constexpr int MC = 4; __VA_ARGS__; } break;    \
    default: { constexpr int MC = 8; __VA_ARGS__; } break;   \
  }

// partial dgamma / dbeta rows of a backward over M rows: one per block of nwv waves x GOAT_LN_RIF rows in flight
int ln_bwd_parts(int M, int nwv) {
  const int nparts = (M + nwv * GOAT_LN_RIF - 1) / (nwv * GOAT_LN_RIF);
  return nparts > GOAT_LN_BWD_PARTS ? GOAT_LN_BWD_PARTS : nparts;
}

// goat_ln_bwd_do's arguments behind its checks, as the kernels take them
struct LnBwdCall {
  hipStream_t st;
  const void *dy, *dy2, *z;
  const float *gamma, *mean, *rstd;
  float p;
  uint64_t seed, offset;
  const uint64_t* rng_dev;
  void *dx, *d_res;
  float *ws, *dgamma, *dbeta;
  const void* dx_add;
  int pre_add, M, H;
  float p_out;
  uint64_t offset_out;
  void* d_post;
  int nparts;
  size_t sm;      // [NWV][2][H] floats of LDS
};

template <typename T, int MC, int RIF, int NWV>
int ln_bwd_launch(const LnBwdCall& c) {
  // rows wider than 1536 (bf16) / 768 (f32) elements: ONE row in flight (two spilled 54 .. 760 registers)
  auto kern = ln_bwd_kernel<T, MC, (MC > 3 ? 1 : RIF), NWV>;
  if (c.sm > 64 * 1024) {
    static size_t attr = 0;      // (one per instantiation: the largest size set so far)
    if (c.sm > attr) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.sm) != hipSuccess)
        return GOAT_E_SHAPE;
      attr = c.sm;
    }
  }
  hipLaunchKernelGGL(kern, dim3(c.nparts), dim3(64 * NWV), c.sm, c.st, (const T*)c.dy, (const T*)c.dy2, (const T*)c.z, c.gamma, c.mean,
                     c.rstd, c.p, c.seed, c.offset, c.rng_dev, (T*)c.dx, (T*)c.d_res, c.ws, c.dgamma, c.dbeta, (const T*)c.dx_add,
                     c.pre_add, c.M, c.H, c.p_out, c.offset_out, (T*)c.d_post);
  return 0;
}

// the 96-VGPR form (ln_bwd768_kernel): same grid, same partial rows, same results
template <int NWV>
int ln_bwd768_launch(const LnBwdCall& c) {
  const bool extra = c.dx_add != nullptr || c.p_out > 0.f || c.d_post != nullptr;
  return bool_dispatch(extra, [&](auto x) {
    return bool_dispatch(c.p > 0.f, [&](auto drop) {
      return bool_dispatch(c.dy2 != nullptr, [&](auto two) {
        constexpr bool DROP = decltype(drop)::value, DY2 = decltype(two)::value;
        hipLaunchKernelGGL((decltype(x)::value ? ln_bwd768x_kernel<NWV, GOAT_LN_RIF, DROP, DY2> : ln_bwd768_kernel<NWV, GOAT_LN_RIF, DROP, DY2>),
                           dim3(c.nparts), dim3(64 * NWV), c.sm + 768 * sizeof(float), c.st, (const bf16_t*)c.dy, (const bf16_t*)c.dy2,
                           (const bf16_t*)c.z, c.gamma, c.mean, c.rstd, c.p, c.seed, c.offset, c.rng_dev, (bf16_t*)c.dx, (bf16_t*)c.d_res,
                           c.ws, c.dgamma, c.dbeta, (const bf16_t*)c.dx_add, c.pre_add, c.M, c.p_out, c.offset_out, (bf16_t*)c.d_post);
        return 0;
      });
    });
  });
}

}  // namespace

extern "C" int goat_ln_fwd_do(void* stream, int dtype, const void* x, const void* residual, const float* gamma,
                              const float* beta, float eps, float p, uint64_t seed, uint64_t offset,
                              const uint64_t* rng_dev, void* y, void* z_out, float* mean, float* rstd, int M, int H, float p_out,
                              uint64_t offset_out, const void* post_add) {
  if (!x || !gamma || !beta || !y || !mean || !rstd) return GOAT_E_ARG;
  if (M <= 0 || !(p_out >= 0.f && p_out < 1.f)) return GOAT_E_SHAPE;
  if ((residual || p > 0.f) && !z_out) return GOAT_E_ARG;
  dim3 grid((M + 3) / 4);
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    if (int e = ln_check<T>(H)) return e;
    GOAT_LN_DISPATCH(T, H, hipLaunchKernelGGL((ln_fwd_kernel<T, MC>), grid, dim3(256), 0, ST(stream), (const T*)x, (const T*)residual, gamma,
                                              beta, eps, p, seed, offset, rng_dev, (T*)y, (T*)z_out, mean, rstd, M, H, p_out, offset_out,
                                              (const T*)post_add));
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_ln_fwd(void* stream, int dtype, const void* x, const void* residual, const float* gamma,
                           const float* beta, float eps, float p, uint64_t seed, uint64_t offset,
                           const uint64_t* rng_dev, void* y, void* z_out, float* mean, float* rstd, int M, int H) {
  return goat_ln_fwd_do(stream, dtype, x, residual, gamma, beta, eps, p, seed, offset, rng_dev, y, z_out, mean, rstd, M, H, 0.f, 0,
                        nullptr);
}

extern "C" int goat_ln_bwd_ws_floats(int H) { return GOAT_LN_BWD_PARTS * 2 * H; }

// partial rows written by goat_ln_bwd(..., accumulate = 2)
extern "C" int goat_ln_bwd_nparts(int M) { return ln_bwd_parts(M, GOAT_LN_BWD_WAVES); }

extern "C" int goat_ln_reduce_batched(void* stream, const goat_ln_partial* entries, int n, int H) {
  if (!entries || n < 0 || H <= 0) return GOAT_E_ARG;
  // same destination -> adjacent (stable: call order kept inside a run); consecutive launches on one stream are ordered, so a run
  // cut by the 64-entry limit is still summed by one writer at a time
  std::vector<goat_ln_partial> sorted(entries, entries + n);
  std::stable_sort(sorted.begin(), sorted.end(), [](const goat_ln_partial& x, const goat_ln_partial& y) {
    return reinterpret_cast<uintptr_t>(x.dgamma) < reinterpret_cast<uintptr_t>(y.dgamma);
  });
  for (int k = 1; k < n; ++k)
    if (sorted[k].dgamma == sorted[k - 1].dgamma && sorted[k].dbeta != sorted[k - 1].dbeta) return GOAT_E_ARG;
  for (int first = 0; first < n; first += 64) {
    LnReduceArgs a;
    a.n = n - first < 64 ? n - first : 64;
    a.H = H;
    for (int k = 0; k < a.n; ++k) {
      const goat_ln_partial& e = sorted[first + k];
      if (!e.ws || !e.dgamma || !e.dbeta || e.nparts <= 0) return GOAT_E_ARG;
      a.e[k].ws = e.ws; a.e[k].dgamma = e.dgamma; a.e[k].dbeta = e.dbeta; a.e[k].nparts = e.nparts; a.e[k].pad = 0;
    }
    hipLaunchKernelGGL(ln_reduce_batched_kernel, dim3((2 * H + 15) / 16, a.n), dim3(256), 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int goat_ln_bwd_do(void* stream, int dtype, const void* dy, const void* dy2, const void* z, const float* gamma,
                              const float* mean, const float* rstd, float p, uint64_t seed, uint64_t offset,
                              const uint64_t* rng_dev, void* dx, void* d_res, float* dgamma, float* dbeta, float* ws,
                              int M, int H, int accumulate, const void* dx_add, float p_out, uint64_t offset_out, void* d_post) {
  if (!dy || !z || !gamma || !mean || !rstd || !dgamma || !dbeta) return GOAT_E_ARG;
  if (M <= 0 || !(p_out >= 0.f && p_out < 1.f)) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    if (int e = ln_check<T>(H)) return e;      // (in front of the clearing launch below: a refused call leaves dgamma / dbeta as they were)
    // deterministic mode (ws): 4-wave blocks, up to 512 per-block partial rows reduced by a second kernel (round 1).
    // atomic mode: GOAT_LN_BWD_WAVES-wave blocks (default 4) — with more waves fewer blocks contend for the 2*H gradient words
    // (profiles/round2_ln_bench.txt), but the block's LDS no longer fits beside a GEMM workgroup (see GOAT_LN_BWD_WAVES)
    // accumulate == 2: the per-block partials stay in ws (goat_ln_bwd_nparts(M) rows of 2*H floats) and the caller reduces them
    // later with goat_ln_reduce_batched — the column reduction was 6.8 of the kernel's 15.8 us at 3840 rows (profiles/round2_ln_bench.txt)
    const int pre_add = (accumulate & 4) ? 1 : 0;      // GOAT_LN_ADD_BEFORE: dx_add joins the gradient of the pre-norm sum (see goat_hip.h)
    const int acc = accumulate & 3;
    const bool defer = acc == 2;
    if (defer && ws == nullptr) return GOAT_E_ARG;
    const bool det = ws != nullptr && !defer;
    const int nwv = det ? 4 : GOAT_LN_BWD_WAVES;
    LnBwdCall c;      // (by name: most fields are pointers of one type)
    c.st = ST(stream); c.dy = dy; c.dy2 = dy2; c.z = z; c.gamma = gamma; c.mean = mean; c.rstd = rstd;
    c.p = p; c.seed = seed; c.offset = offset; c.rng_dev = rng_dev; c.dx = dx; c.d_res = d_res;
    c.ws = ws; c.dgamma = dgamma; c.dbeta = dbeta; c.dx_add = dx_add; c.pre_add = pre_add; c.M = M; c.H = H;
    c.p_out = p_out; c.offset_out = offset_out; c.d_post = d_post;
    c.nparts = ln_bwd_parts(M, nwv); c.sm = (size_t)nwv * 2 * H * sizeof(float);
    if (c.sm > 160 * 1024) return GOAT_E_SHAPE;
    if (!det && !defer && !acc) {      // atomic mode writes by accumulation: an overwrite clears the two vectors first.
      // A KERNEL, not hipMemsetAsync: captured into a hipGraph (ROCm 7.2) the two memset nodes left every fourth float of the
      // vectors uncleared in a graph with parallel branches (found by tests/test_rollout_gpu.py: garbage in a LayerNorm weight
      // gradient of a replayed episode; GOAT_LN_DETERMINISTIC=1, which does not clear, was clean).
      hipLaunchKernelGGL(zero2_kernel, dim3((H + 255) / 256), dim3(256), 0, c.st, dgamma, dbeta, H);
    }
    const bool row768 = dt.id == GOAT_BF16 && H == 768 && GOAT_LN_BWD768 && (int64_t)M * H * 2 < (1ll << 31) && !getenv("GOAT_LN_BWD_GENERIC");
    if (int e = bool_dispatch(det, [&](auto d) -> int {
          constexpr int NWV = decltype(d)::value ? 4 : GOAT_LN_BWD_WAVES;
          if (row768) return ln_bwd768_launch<NWV>(c);
          GOAT_LN_DISPATCH(T, H, if (int e = ln_bwd_launch<T, MC, (sizeof(T) == 2 ? GOAT_LN_RIF : 2), NWV>(c)) return e);
          return 0;
        }))
      return e;
    GOAT_LAUNCH_CHECK();
    if (det) {
      hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((2 * H + 15) / 16), dim3(256), 0, c.st, ws, dgamma, dbeta, c.nparts, H, acc);
      GOAT_LAUNCH_CHECK();
    }
    return 0;
  });
}

extern "C" int goat_ln_bwd(void* stream, int dtype, const void* dy, const void* dy2, const void* z, const float* gamma,
                           const float* mean, const float* rstd, float p, uint64_t seed, uint64_t offset,
                           const uint64_t* rng_dev, void* dx, void* d_res, float* dgamma, float* dbeta, float* ws,
                           int M, int H, int accumulate, const void* dx_add) {
  return goat_ln_bwd_do(stream, dtype, dy, dy2, z, gamma, mean, rstd, p, seed, offset, rng_dev, dx, d_res, dgamma, dbeta, ws, M, H,
                        accumulate, dx_add, 0.f, 0, nullptr);
}
