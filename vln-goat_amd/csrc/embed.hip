// Input assembly of the encoders (ops_embed): adaptive panorama fusion, gather / segment-mean, embedding tables.
#include <cstdlib>
#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------ pano fusion
// one block (4 waves) per panorama; V <= 64 slots.  score_v = tanh(x_v·a + a0); w = softmax_v(score)
template <typename T>
__global__ __launch_bounds__(256) void pano_fusion_fwd_generic(const T* __restrict__ x, const float* __restrict__ a,
                                                              const float* __restrict__ a0, T* __restrict__ fused,
                                                              float* __restrict__ wsave, int V, int H) {
  __shared__ float sc[64];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* xb = x + (int64_t)n * V * H;
  for (int v = wave; v < V; v += 4) {
    float s = 0.f;
    for (int i = lane; i < H; i += 64) s += to_f(xb[(int64_t)v * H + i]) * a[i];
    s = wave_sum(s);
    if (lane == 0) sc[v] = tanhf(s + a0[0]);
  }
  __syncthreads();
  if (wave == 0) {
    float v = lane < V ? sc[lane] : -INFINITY;
    float m = wave_max(v);
    float e = lane < V ? __expf(v - m) : 0.f;
    float l = wave_sum(e);
    if (lane < V) { sc[lane] = e / l; wsave[(int64_t)n * V + lane] = e / l; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += 256) {
    float s = 0.f;
    for (int v = 0; v < V; ++v) s += sc[v] * to_f(xb[(int64_t)v * H + i]);
    fused[(int64_t)n * H + i] = from_f<T>(s);
  }
}

// backward: df[H] given.  g_v = x_v·df ; d(softmax in)_v = w_v (g_v - sum_u w_u g_u) ;
// dscore_v = d(softmax in)_v * (1 - tanh^2(x_v·a + a0)) ; dx_v = w_v*df + dscore_v * a
template <typename T>
__global__ __launch_bounds__(256) void pano_fusion_bwd_generic(const T* __restrict__ x, const float* __restrict__ a,
                                                              const float* __restrict__ a0,
                                                              const float* __restrict__ wsave, const T* __restrict__ dfused,
                                                              T* __restrict__ dx, float* __restrict__ da,
                                                              float* __restrict__ da0, int V, int H) {
  __shared__ float gl[64], tl[64], dsc[64];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* xb = x + (int64_t)n * V * H;
  const T* df = dfused + (int64_t)n * H;
  for (int v = wave; v < V; v += 4) {
    float g = 0.f, s = 0.f;
    for (int i = lane; i < H; i += 64) {
      const float xv = to_f(xb[(int64_t)v * H + i]);
      g += xv * to_f(df[i]);
      s += xv * a[i];
    }
    g = wave_sum(g);
    s = wave_sum(s);
    if (lane == 0) { gl[v] = g; tl[v] = tanhf(s + a0[0]); }
  }
  __syncthreads();
  if (wave == 0) {
    const float w = lane < V ? wsave[(int64_t)n * V + lane] : 0.f;
    const float g = lane < V ? gl[lane] : 0.f;
    const float wg = wave_sum(w * g);
    if (lane < V) dsc[lane] = w * (g - wg) * (1.f - tl[lane] * tl[lane]);
  }
  __syncthreads();
  for (int v = wave; v < V; v += 4) {
    const float w = wsave[(int64_t)n * V + v];
    const float d = dsc[v];
    for (int i = lane; i < H; i += 64)
      dx[((int64_t)n * V + v) * H + i] = from_f<T>(w * to_f(df[i]) + d * a[i]);
  }
  for (int i = threadIdx.x; i < H; i += 256) {
    float s = 0.f;
    for (int v = 0; v < V; ++v) s += dsc[v] * to_f(xb[(int64_t)v * H + i]);
    atomicAdd(da + i, s);
  }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int v = 0; v < V; ++v) s += dsc[v];
    atomicAdd(da0, s);
  }
}

// Single-pass versions (H % EPC == 0, H <= 64*EPC*MAXC): one block of 8 waves per panorama, wave w keeps rows w, w+8, ... (<= 8 of
// them) in registers as 16-byte chunks, so x is read once (the generic kernels above read it twice with 2-byte loads: 70 / 82 us
// for 240 panoramas of 36 x 768 against ~8 us here).  Cross-wave sums (the fused vector, da) go through LDS.
constexpr int PF_NW = 8, PF_RMAX = 8;
template <typename T, int MAXC>
__global__ __launch_bounds__(64 * PF_NW) void pano_fusion_fwd_kernel(const T* __restrict__ x, const float* __restrict__ a,
                                                                     const float* __restrict__ a0, T* __restrict__ fused,
                                                                     float* __restrict__ wsave, int V, int H) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float psm[];   // [PF_NW][H]
  __shared__ float sc[64];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = H / EPC;
  const T* xb = x + (int64_t)n * V * H;
  Chunk<T> xv[PF_RMAX][MAXC];
#pragma unroll
  for (int r = 0; r < PF_RMAX; ++r) {
    const int v = wave + PF_NW * r;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (v < V && c < nchunk) xv[r][i].load(xb + (int64_t)v * H + c * EPC);
      else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) xv[r][i].v[e] = 0.f;
      }
    }
  }
  float av[MAXC][EPC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
#pragma unroll
    for (int e = 0; e < EPC; ++e) av[i][e] = c < nchunk ? a[c * EPC + e] : 0.f;
  }
  const float bias = a0[0];
#pragma unroll
  for (int r = 0; r < PF_RMAX; ++r) {
    const int v = wave + PF_NW * r;
    if (v < V) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < MAXC; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) s += xv[r][i].v[e] * av[i][e];
      s = wave_sum(s);
      if (lane == 0) sc[v] = tanhf(s + bias);
    }
  }
  __syncthreads();
  if (wave == 0) {
    const float v = lane < V ? sc[lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = lane < V ? __expf(v - m) : 0.f;
    const float l = wave_sum(e);
    if (lane < V) { sc[lane] = e / l; wsave[(int64_t)n * V + lane] = e / l; }
  }
  __syncthreads();
  float acc[MAXC][EPC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[i][e] = 0.f;
#pragma unroll
  for (int r = 0; r < PF_RMAX; ++r) {
    const int v = wave + PF_NW * r;
    if (v < V) {
      const float w = sc[v];
#pragma unroll
      for (int i = 0; i < MAXC; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[i][e] += w * xv[r][i].v[e];
    }
  }
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) psm[wave * H + c * EPC + e] = acc[i][e];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += 64 * PF_NW) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < PF_NW; ++w) s += psm[w * H + i];
    fused[(int64_t)n * H + i] = from_f<T>(s);
  }
}

template <typename T, int MAXC>
__global__ __launch_bounds__(64 * PF_NW) void pano_fusion_bwd_kernel(const T* __restrict__ x, const float* __restrict__ a,
                                                                     const float* __restrict__ a0,
                                                                     const float* __restrict__ wsave, const T* __restrict__ dfused,
                                                                     T* __restrict__ dx, float* __restrict__ da,
                                                                     float* __restrict__ da0, int V, int H) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float psm[];   // [PF_NW][H]
  __shared__ float gl[64], tl[64], dsc[64], wl[64];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = H / EPC;
  const T* xb = x + (int64_t)n * V * H;
  Chunk<T> xv[PF_RMAX][MAXC];
#pragma unroll
  for (int r = 0; r < PF_RMAX; ++r) {
    const int v = wave + PF_NW * r;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (v < V && c < nchunk) xv[r][i].load(xb + (int64_t)v * H + c * EPC);
      else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) xv[r][i].v[e] = 0.f;
      }
    }
  }
  float av[MAXC][EPC];
  Chunk<T> dfv[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) dfv[i].load(dfused + (int64_t)n * H + c * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      av[i][e] = c < nchunk ? a[c * EPC + e] : 0.f;
      if (c >= nchunk) dfv[i].v[e] = 0.f;
    }
  }
  const float bias = a0[0];
#pragma unroll
  for (int r = 0; r < PF_RMAX; ++r) {
    const int v = wave + PF_NW * r;
    if (v < V) {
      float g = 0.f, s = 0.f;
#pragma unroll
      for (int i = 0; i < MAXC; ++i)
#pragma unroll
        for (int e = 0; e < EPC; ++e) { g += xv[r][i].v[e] * dfv[i].v[e]; s += xv[r][i].v[e] * av[i][e]; }
      g = wave_sum(g);
      s = wave_sum(s);
      if (lane == 0) { gl[v] = g; tl[v] = tanhf(s + bias); }
    }
  }
  __syncthreads();
  if (wave == 0) {
    const float w = lane < V ? wsave[(int64_t)n * V + lane] : 0.f;
    const float g = lane < V ? gl[lane] : 0.f;
    const float wg = wave_sum(w * g);
    const float d = w * (g - wg) * (1.f - tl[lane < V ? lane : 0] * tl[lane < V ? lane : 0]);
    if (lane < V) { dsc[lane] = d; wl[lane] = w; }
    const float tot = wave_sum(lane < V ? d : 0.f);
    if (lane == 0) atomicAdd(da0, tot);
  }
  __syncthreads();
  float acc[MAXC][EPC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[i][e] = 0.f;
#pragma unroll
  for (int r = 0; r < PF_RMAX; ++r) {
    const int v = wave + PF_NW * r;
    if (v < V) {
      const float w = wl[v], d = dsc[v];
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = lane + 64 * i;
        Chunk<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          o.v[e] = w * dfv[i].v[e] + d * av[i][e];
          acc[i][e] += d * xv[r][i].v[e];
        }
        if (c < nchunk) o.store_stream(dx + ((int64_t)n * V + v) * H + c * EPC);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) psm[wave * H + c * EPC + e] = acc[i][e];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += 64 * PF_NW) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < PF_NW; ++w) s += psm[w * H + i];
    atomicAdd(da + i, s);
  }
}

// ------------------------------------------------------------------------------------ gather / segment mean
template <typename T>
__global__ __launch_bounds__(256) void gather_fwd_kernel(const T* __restrict__ src, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ start, const float* __restrict__ scale,
                                                         const float* __restrict__ tok_w, T* __restrict__ out, int n_out, int H) {
  constexpr int EPC = DT<T>::EPC;
  const int nchunk = H / EPC;
  const int64_t total = (int64_t)n_out * nchunk;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / nchunk), c = (int)(t % nchunk);
    Chunk<T> acc;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc.v[e] = 0.f;
    for (int j = start[i]; j < start[i + 1]; ++j) {
      const int s = idx[j];
      if (s >= 0) {
        Chunk<T> v;
        v.load(src + (int64_t)s * H + c * EPC);
        const float w = tok_w ? tok_w[j] : 1.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc.v[e] += v.v[e] * w;
      }
    }
    const float sc = scale ? scale[i] : 1.f;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc.v[e] *= sc;
    acc.store(out + (int64_t)i * H + c * EPC);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gather_bwd_kernel(const T* __restrict__ dout, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ start, const float* __restrict__ scale,
                                                         float* __restrict__ dsrc, int n_out, int H) {
  constexpr int EPC = DT<T>::EPC;
  const int nchunk = H / EPC;
  const int64_t total = (int64_t)n_out * nchunk;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / nchunk), c = (int)(t % nchunk);
    if (start[i] == start[i + 1]) continue;
    Chunk<T> g;
    g.load(dout + (int64_t)i * H + c * EPC);
    const float sc = scale ? scale[i] : 1.f;
    for (int j = start[i]; j < start[i + 1]; ++j) {
      const int s = idx[j];
      if (s >= 0) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) atomicAdd(dsrc + (int64_t)s * H + c * EPC + e, g.v[e] * sc);
      }
    }
  }
}

// ------------------------------------------------------------------------------------ embedding tables
// out[r] = word[ids[r]] (+ type[tids ? tids[r] : 0]) (+ pos[r % L]) — the three lookups and two adds of
// BertEmbeddings (P/model/Bert_backbone.py:98-113; position ids are arange(L)) in one pass; tables are the f32 masters.
template <typename T>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const float* __restrict__ word, const int64_t* __restrict__ ids,
                                                        const float* __restrict__ type_tab, const int64_t* __restrict__ tids,
                                                        const float* __restrict__ pos_tab, int L, T* __restrict__ out,
                                                        int rows, int H, int vocab, int* __restrict__ err) {
  constexpr int EPC = DT<T>::EPC;
  const int nchunk = H / EPC;
  const int64_t total = (int64_t)rows * nchunk;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(t / nchunk), c = (int)(t % nchunk);
    int64_t id = ids[r];
    if (id < 0 || id >= vocab) {  // torch raises on an out-of-range index; flag it and read row 0
      if (err) atomicOr(err, 1);
      id = 0;
    }
    float acc[EPC];
    {
      const float* w = word + id * H + c * EPC;
#pragma unroll
      for (int e = 0; e < EPC; e += 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(w + e);
        acc[e] = v[0]; acc[e + 1] = v[1]; acc[e + 2] = v[2]; acc[e + 3] = v[3];
      }
    }
    if (type_tab) {
      const float* w = type_tab + (tids ? tids[r] : 0) * H + c * EPC;
#pragma unroll
      for (int e = 0; e < EPC; e += 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(w + e);
        acc[e] += v[0]; acc[e + 1] += v[1]; acc[e + 2] += v[2]; acc[e + 3] += v[3];
      }
    }
    if (pos_tab) {
      const float* w = pos_tab + (int64_t)(r % L) * H + c * EPC;
#pragma unroll
      for (int e = 0; e < EPC; e += 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(w + e);
        acc[e] += v[0]; acc[e + 1] += v[1]; acc[e + 2] += v[2]; acc[e + 3] += v[3];
      }
    }
    Chunk<T> o;
#pragma unroll
    for (int e = 0; e < EPC; ++e) o.v[e] = acc[e];
    o.store(out + (int64_t)r * H + c * EPC);
  }
}

// scatter-add of d(out) into the (pre-zeroed) f32 table gradients.  Rows whose id equals the table's
// padding index contribute nothing (nn.Embedding(padding_idx=…) semantics, Bert_backbone.py:85-87 — this
// also zeroes the gradient of position row `pos_pad`, as in the reference).
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                        const int64_t* __restrict__ tids, int L, float* __restrict__ dword,
                                                        float* __restrict__ dtype_tab, float* __restrict__ dpos, int rows,
                                                        int H, int vocab, int word_pad, int pos_pad) {
  // one wave per row; lane l owns columns l, l+64, ...: every atomic instruction of a wave covers 256 contiguous
  // bytes of one table row (the memory-side atomic units coalesce those; 32-B-strided lanes do not).
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int nwave = gridDim.x * (blockDim.x >> 6);
  for (int r = wave; r < rows; r += nwave) {
    const int64_t id = ids[r];
    float* dw = (dword && id >= 0 && id < vocab && id != word_pad) ? dword + id * H : nullptr;
    float* dt = (dtype_tab && tids) ? dtype_tab + tids[r] * H : nullptr;
    const int l = r % L;
    float* dp = (dpos && l != pos_pad) ? dpos + (int64_t)l * H : nullptr;
    if (!dw && !dt && !dp) continue;
    const T* g = dout + (int64_t)r * H;
    for (int c = lane; c < H; c += 64) {
      const float v = to_f(g[c]);
      if (dw) atomicAdd(dw + c, v);
      if (dt) atomicAdd(dt + c, v);
      if (dp) atomicAdd(dp + c, v);
    }
  }
}

// Small tables (nav-type, step-id, object-name embeddings: 3..64 rows): every token row lands on a handful of table rows, so the
// per-element atomics of the kernel above serialise on the same words (109 us for 8960 rows into a 3-row table).  Here a block
// owns 64 columns x a chunk of token rows, accumulates in LDS ([row phase][table row][column], one owner per word) and issues one
// atomic per table word and block.
constexpr int ES_MAXV = 64, ES_ROWS = 256;
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_small_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                              float* __restrict__ dtab, int rows, int H, int vocab, int pad_id) {
  extern __shared__ float es[];      // [4][vocab][64]
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  for (int i = threadIdx.x; i < 4 * vocab * 64; i += 256) es[i] = 0.f;
  __syncthreads();
  const int r0 = blockIdx.y * ES_ROWS, r1 = min(rows, r0 + ES_ROWS);
  if (c < H)
    for (int r = r0 + ph; r < r1; r += 4) {
      const int64_t id = ids[r];
      if (id < 0 || id >= vocab || id == pad_id) continue;
      es[(ph * vocab + (int)id) * 64 + lane] += to_f(dout[(int64_t)r * H + c]);
    }
  __syncthreads();
  for (int i = threadIdx.x; i < vocab * 64; i += 256) {
    const int v = i >> 6, l = i & 63;
    const float t = es[(0 * vocab + v) * 64 + l] + es[(1 * vocab + v) * 64 + l] + es[(2 * vocab + v) * 64 + l] + es[(3 * vocab + v) * 64 + l];
    if (t != 0.f && blockIdx.x * 64 + l < H) atomicAdd(dtab + (int64_t)v * H + blockIdx.x * 64 + l, t);
  }
}

// grid of the kernels that give a thread one 16-byte chunk of rows x H at a time (at most 4096 blocks); 0 if H is no whole chunks
int row_chunk_blocks(int dtype, int rows, int H) {
  const int epc = dtype == GOAT_BF16 ? 8 : 4;
  if (H % epc) return 0;
  const int blocks = (int)(((int64_t)rows * (H / epc) + 255) / 256);
  return blocks > 4096 ? 4096 : blocks;
}

}  // namespace

extern "C" int goat_pano_fusion_fwd(void* stream, int dtype, const void* x, const float* a, const float* a0, void* fused,
                                    float* wsave, int N, int V, int H) {
  if (!x || !a || !a0 || !fused || !wsave) return GOAT_E_ARG;
  if (N <= 0 || V <= 0 || V > 64 || H <= 0) return GOAT_E_SHAPE;
  size_t sm = (size_t)PF_NW * H * sizeof(float);
#ifdef GOAT_PANO_GENERIC
  sm = 1 << 30;
#endif
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    constexpr int MC = sizeof(T) == 2 ? 2 : 3;      // 16-byte chunks per lane of the register kernel: H <= 1024 bf16, 768 f32
    if (H % dt.EPC == 0 && H <= 64 * dt.EPC * MC && sm <= 64 * 1024)
      hipLaunchKernelGGL((pano_fusion_fwd_kernel<T, MC>), dim3(N), dim3(64 * PF_NW), sm, ST(stream), (const T*)x, a, a0, (T*)fused, wsave, V, H);
    else
      hipLaunchKernelGGL(pano_fusion_fwd_generic<T>, dim3(N), dim3(256), 0, ST(stream), (const T*)x, a, a0, (T*)fused, wsave, V, H);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_pano_fusion_bwd(void* stream, int dtype, const void* x, const float* a, const float* a0,
                                    const float* wsave, const void* dfused, void* dx, float* da, float* da0, int N,
                                    int V, int H) {
  if (!x || !a || !a0 || !wsave || !dfused || !dx || !da || !da0) return GOAT_E_ARG;
  if (N <= 0 || V <= 0 || V > 64 || H <= 0) return GOAT_E_SHAPE;
  size_t sm = (size_t)PF_NW * H * sizeof(float);
#ifdef GOAT_PANO_GENERIC
  sm = 1 << 30;
#endif
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    constexpr int MC = sizeof(T) == 2 ? 2 : 3;
    if (H % dt.EPC == 0 && H <= 64 * dt.EPC * MC && sm <= 64 * 1024)
      hipLaunchKernelGGL((pano_fusion_bwd_kernel<T, MC>), dim3(N), dim3(64 * PF_NW), sm, ST(stream), (const T*)x, a, a0, wsave, (const T*)dfused,
                         (T*)dx, da, da0, V, H);
    else
      hipLaunchKernelGGL(pano_fusion_bwd_generic<T>, dim3(N), dim3(256), 0, ST(stream), (const T*)x, a, a0, wsave, (const T*)dfused, (T*)dx, da,
                         da0, V, H);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_gather_segmean_fwd(void* stream, int dtype, const void* src, int64_t src_rows, const int32_t* idx,
                                       const int32_t* start, const float* scale, void* out, int n_out, int H, const float* tok_w) {
  if (!src || !idx || !start || !out) return GOAT_E_ARG;
  if (n_out <= 0 || H <= 0 || src_rows <= 0) return GOAT_E_SHAPE;
  const int blocks = row_chunk_blocks(dtype, n_out, H);
  if (!blocks) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(gather_fwd_kernel<T>, dim3(blocks), dim3(256), 0, ST(stream), (const T*)src, idx, start, scale, tok_w, (T*)out, n_out, H);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_gather_segmean_bwd(void* stream, int dtype, const void* dout, const int32_t* idx,
                                       const int32_t* start, const float* scale, float* dsrc32, int n_out, int H) {
  if (!dout || !idx || !start || !dsrc32) return GOAT_E_ARG;
  if (n_out <= 0 || H <= 0) return GOAT_E_SHAPE;
  const int blocks = row_chunk_blocks(dtype, n_out, H);
  if (!blocks) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(gather_bwd_kernel<T>, dim3(blocks), dim3(256), 0, ST(stream), (const T*)dout, idx, start, scale, dsrc32, n_out, H);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_embed_fwd(void* stream, int dtype, const float* word, const int64_t* ids, const float* type_tab,
                             const int64_t* type_ids, const float* pos_tab, int L, void* out, int rows, int H, int vocab,
                             int* err_flag) {
  if (!word || !ids || !out) return GOAT_E_ARG;
  if (rows <= 0 || H <= 0 || vocab <= 0 || (pos_tab && L <= 0)) return GOAT_E_SHAPE;
  const int blocks = row_chunk_blocks(dtype, rows, H);
  if (!blocks) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(embed_fwd_kernel<T>, dim3(blocks), dim3(256), 0, ST(stream), word, ids, type_tab, type_ids, pos_tab, L, (T*)out, rows, H,
                       vocab, err_flag);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_embed_bwd(void* stream, int dtype, const void* dout, const int64_t* ids, const int64_t* type_ids,
                             int L, float* dword, float* dtype_tab, float* dpos, int rows, int H, int vocab, int word_pad,
                             int pos_pad) {
  if (!dout || !ids) return GOAT_E_ARG;
  if (rows <= 0 || H <= 0 || vocab <= 0 || (dpos && L <= 0)) return GOAT_E_SHAPE;
  const int epc = dtype == GOAT_BF16 ? 8 : 4;
  if (H % epc) return GOAT_E_SHAPE;
  static const bool es_off = getenv("GOAT_NO_EMBED_SMALL") != nullptr;      // (diagnostics: A/B)
  if (!es_off && dword && !dtype_tab && !dpos && vocab <= ES_MAXV && rows >= 512) {      // single small table: LDS accumulation per block
    dim3 grid((H + 63) / 64, (rows + ES_ROWS - 1) / ES_ROWS);
    const size_t sm = (size_t)4 * vocab * 64 * sizeof(float);
    return dtype_dispatch(dtype, [&](auto dt) -> int {
      typedef GOAT_DT_TYPE(dt) T;
      hipLaunchKernelGGL(embed_bwd_small_kernel<T>, grid, dim3(256), sm, ST(stream), (const T*)dout, ids, dword, rows, H, vocab, word_pad);
      GOAT_LAUNCH_CHECK();
      return 0;
    });
  }
  int blocks = (rows + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(embed_bwd_kernel<T>, dim3(blocks), dim3(256), 0, ST(stream), (const T*)dout, ids, type_ids, L, dword, dtype_tab, dpos,
                       rows, H, vocab, word_pad, pos_pad);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}
