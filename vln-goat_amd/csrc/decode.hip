// goat_attn_decode_fwd / goat_decode_select: one step of KV-cached decoding (the speaker's back-translation loop) with the step's
// position in DEVICE memory, so that the step is a fixed-shape computation a hipGraph can replay.
//
// goat_attn_decode_fwd — one block of four waves per (sample, head).  The work is tiny (at most 512 keys x 64 columns) and the point is
// latency, so everything is one launch and no workgroup ever talks to another:
//   1. the block copies ITS head's 64 K and 64 V columns of the new row into cache[b, t] (t = *pos_dev); nobody else reads or writes them;
//   2. scores: a thread per key (two passes cover 512), the whole 64-wide K row in 16-byte loads against the query held in LDS
//      (a broadcast read); key t is taken from KVnew itself, so the kernel never reads back what it has just stored;
//   3. softmax over the keys <= t through two block reductions; the probabilities (dropout applied) go to LDS;
//   4. P·V: the threads are (key group, 16-byte column chunk) pairs, consecutive threads cover one V row (coalesced), each walks its
//      keys with a stride of the group count; the groups are added through LDS in a fixed order (bitwise reproducible).
// Keys > t are never loaded: the cache tail may hold anything.
//
// goat_decode_select — ONE block of sixteen waves for all rows (a wave per row, rows strided over the waves): with a single workgroup
// the increment of *pos_dev and the count of live rows need no inter-workgroup protocol.  Arg-max ties go to the LOWEST index: a lane
// scans its columns in increasing order and replaces its best only by a strictly greater value, and the cross-lane reduction prefers
// the lower index among equal values.  NaN logits are treated as -inf.
#include <limits.h>
#include "common.hpp"

namespace {

constexpr int DEC_HD = 64;
constexpr int DEC_MAXL = 512;
constexpr int DEC_THREADS = 256;
constexpr int SEL_WAVES = 16;

struct DecodeArgs {
  const void *Q, *KVnew;
  void *cache, *O;
  int64_t c_rs, c_bs;
  const float* kmask;
  const int32_t* pos;
  int B, nh, Lmax;
  float scale, p;
  uint64_t seed, offset;
  const uint64_t* rng_dev;
};

template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_kernel(DecodeArgs a) {
  constexpr int NE = DT<T>::EPC;              // elements per 16-byte chunk
  constexpr int CPR = DEC_HD / NE;            // chunks per head row (bf16 8, f32 16)
  constexpr int KG = DEC_THREADS / CPR;       // key groups of the P·V phase (bf16 32, f32 16)
  __shared__ float qs[DEC_HD];
  __shared__ float prob[DEC_MAXL];
  __shared__ __attribute__((aligned(16))) float red[KG * DEC_HD];
  __shared__ float wbuf[DEC_THREADS / 64];

  const int t = *a.pos;
  if (t < 0 || t >= a.Lmax) return;           // (block-uniform) a position outside the cache: touch nothing

  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.nh, h = blockIdx.x % a.nh;
  const int H = a.nh * DEC_HD;
  const T* q = reinterpret_cast<const T*>(a.Q) + (int64_t)b * H + h * DEC_HD;
  const T* kvn = reinterpret_cast<const T*>(a.KVnew) + (int64_t)b * 2 * H + h * DEC_HD;      // K columns of this head; V at + H
  T* cb = reinterpret_cast<T*>(a.cache) + (int64_t)b * a.c_bs + h * DEC_HD;

  if (tid < 2 * CPR) {                        // append: this head's K and V columns of the new row
    const int kv = tid / CPR, cc = tid % CPR;
    *reinterpret_cast<uint4*>(cb + (int64_t)t * a.c_rs + kv * H + cc * NE) = *reinterpret_cast<const uint4*>(kvn + kv * H + cc * NE);
  }
  if (tid < DEC_HD) qs[tid] = to_f(q[tid]);
  __syncthreads();

  const float* kmask = a.kmask ? a.kmask + (int64_t)b * a.Lmax : nullptr;
  float s[DEC_MAXL / DEC_THREADS];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < DEC_MAXL / DEC_THREADS; ++i) {
    const int k = tid + i * DEC_THREADS;
    float v = -INFINITY;
    if (k <= t) {
      const T* row = (k == t) ? kvn : cb + (int64_t)k * a.c_rs;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < CPR; ++c) {
        Chunk<T> ch;
        ch.load(row + c * NE);
#pragma unroll
        for (int e = 0; e < NE; ++e) acc = fmaf(ch.v[e], qs[c * NE + e], acc);
      }
      v = acc * a.scale;
      if (kmask) v += kmask[k];
    }
    s[i] = v;
    m = fmaxf(m, v);
  }
  m = block_reduce<true, DEC_THREADS / 64>(m, wbuf);
  const float msafe = (m == -INFINITY) ? 0.f : m;       // every visible key at -inf: exp(-inf - 0) = 0, never inf - inf
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < DEC_MAXL / DEC_THREADS; ++i) {
    s[i] = (tid + i * DEC_THREADS <= t) ? __expf(s[i] - msafe) : 0.f;
    l += s[i];
  }
  l = block_reduce<false, DEC_THREADS / 64>(l, wbuf);
  const float inv = l > 0.f ? 1.f / l : 0.f;

  const bool drop = a.p > 0.f;
  const uint32_t thr = goat_thr16(a.p);
  const float keep_scale = drop ? 1.f / (1.f - a.p) : 1.f;
  const HeadRng rng(a.seed + (a.rng_dev ? *a.rng_dev : 0ull), a.offset, (uint32_t)(b * a.nh + h));
#pragma unroll
  for (int i = 0; i < DEC_MAXL / DEC_THREADS; ++i) {
    const int k = tid + i * DEC_THREADS;
    float pk = s[i] * inv;
    if (drop) pk = rng.keep((uint32_t)k, thr) ? pk * keep_scale : 0.f;
    prob[k] = pk;
  }
  __syncthreads();

  {
    const int g = tid / CPR, cc = tid % CPR;
    float acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.f;
    for (int k = g; k <= t; k += KG) {
      const T* row = ((k == t) ? kvn : cb + (int64_t)k * a.c_rs) + H;
      Chunk<T> ch;
      ch.load(row + cc * NE);
      const float pk = prob[k];
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[e] = fmaf(pk, ch.v[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) red[g * DEC_HD + cc * NE + e] = acc[e];
  }
  __syncthreads();
  if (tid < DEC_HD) {
    float o = 0.f;
#pragma unroll 8
    for (int g = 0; g < KG; ++g) o += red[g * DEC_HD + tid];
    reinterpret_cast<T*>(a.O)[(int64_t)b * H + h * DEC_HD + tid] = from_f<T>(o);
  }
}

struct SelectArgs {
  const float* logits;
  int64_t ld;
  int B, V, Lmax, unk, eos, pad, sampling;
  uint64_t seed, offset;
  const uint64_t* rng_dev;
  int32_t* pos;
  int64_t* words;
  float* kmask;
  uint8_t* ended;
  int32_t* end_step;
  int32_t* n_live;
};

__global__ __launch_bounds__(64 * SEL_WAVES) void decode_select_kernel(SelectArgs a) {
  __shared__ int live[SEL_WAVES];
  const int t = *a.pos;
  if (t < 0 || t + 1 >= a.Lmax) return;       // no column t + 1 to write: touch nothing
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GoatRng rng(a.seed + (a.rng_dev ? *a.rng_dev : 0ull));
  int nlive = 0;
  for (int b = wave; b < a.B; b += SEL_WAVES) {             // (b, was_ended, word: wave-uniform)
    const bool was_ended = a.ended[b] != 0;
    int word = a.pad;
    if (!was_ended) {
      const float* row = a.logits + (int64_t)b * a.ld;
      float best = -INFINITY;
      int idx = INT_MAX;
      for (int c = lane; c < a.V; c += 64) {
        if (c == a.unk) continue;
        float v = row[c];
        if (v != v) v = -INFINITY;
        if (a.sampling) {                                   // Gumbel-max: argmax(logit + G), G = -log(-log(u)), u in (0, 1)
          const uint32_t hbits = rng.pair_bits(a.offset + (uint64_t)b * (uint64_t)a.V + (uint64_t)c);
          // 23 bits + 0.5 is exact in float32: u in [2^-24, 1 - 2^-24], so G is finite (24 bits would round the top value to u = 1)
          const float u = ((float)(hbits >> 9) + 0.5f) * (1.0f / 8388608.0f);
          v -= logf(-logf(u));
        }
        if (idx == INT_MAX || v > best) { best = v; idx = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (oi != INT_MAX && (idx == INT_MAX || ov > best || (ov == best && oi < idx))) { best = ov; idx = oi; }
      }
      word = idx;
    }
    const bool ends = !was_ended && word == a.eos;
    if (lane == 0) {
      a.words[(int64_t)b * a.Lmax + t + 1] = (int64_t)word;
      a.kmask[(int64_t)b * a.Lmax + t + 1] = (word == a.pad) ? -1e9f : 0.f;
      if (ends) {
        a.ended[b] = 1;
        a.end_step[b] = t;
      }
    }
    if (!was_ended && !ends) ++nlive;
  }
  if (lane == 0) live[wave] = nlive;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) n += live[w];
    *a.n_live = n;
    *a.pos = t + 1;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int goat_attn_decode_fwd(void* stream, int dtype, const void* Q, const void* KVnew, void* cache, int64_t c_rs,
                                    int64_t c_bs, void* O, const float* kmask, const int32_t* pos_dev, int B, int nh, int Lmax,
                                    float scale, float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev) {
  if (!Q || !KVnew || !cache || !O || !pos_dev) return GOAT_E_ARG;
  if (dtype != GOAT_F32 && dtype != GOAT_BF16) return GOAT_E_ARG;
  if (!(p >= 0.f && p < 1.f)) return GOAT_E_ARG;
  if (B <= 0 || nh <= 0 || Lmax < 1 || Lmax > DEC_MAXL) return GOAT_E_SHAPE;
  const int epc = dtype == GOAT_BF16 ? 8 : 4;
  if (c_rs < 2 * (int64_t)nh * DEC_HD || (c_rs % epc) != 0 || (c_bs % epc) != 0) return GOAT_E_SHAPE;
  if (!aligned16(Q) || !aligned16(KVnew) || !aligned16(cache) || !aligned16(O)) return GOAT_E_SHAPE;
  DecodeArgs a = {};
  a.Q = Q; a.KVnew = KVnew; a.cache = cache; a.O = O;
  a.c_rs = c_rs; a.c_bs = c_bs; a.kmask = kmask; a.pos = pos_dev;
  a.B = B; a.nh = nh; a.Lmax = Lmax; a.scale = scale; a.p = p; a.seed = seed; a.offset = offset; a.rng_dev = rng_dev;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    hipLaunchKernelGGL(attn_decode_kernel<GOAT_DT_TYPE(dt)>, dim3(B * nh), dim3(DEC_THREADS), 0, ST(stream), a);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_decode_select(void* stream, const float* logits, int64_t ld, int B, int V, int Lmax, int unk, int eos, int pad,
                                  int sampling, uint64_t seed, uint64_t offset, const uint64_t* rng_dev, int32_t* pos_dev,
                                  int64_t* words, float* kmask, uint8_t* ended, int32_t* end_step, int32_t* n_live) {
  if (!logits || !pos_dev || !words || !kmask || !ended || !end_step || !n_live) return GOAT_E_ARG;
  if (B <= 0 || V < 2 || ld < V || Lmax < 2) return GOAT_E_SHAPE;
  SelectArgs a = {};
  a.logits = logits; a.ld = ld; a.B = B; a.V = V; a.Lmax = Lmax; a.unk = unk; a.eos = eos; a.pad = pad; a.sampling = sampling;
  a.seed = seed; a.offset = offset; a.rng_dev = rng_dev; a.pos = pos_dev;
  a.words = words; a.kmask = kmask; a.ended = ended; a.end_step = end_step; a.n_live = n_live;
  hipLaunchKernelGGL(decode_select_kernel, dim3(1), dim3(64 * SEL_WAVES), 0, ST(stream), a);
  GOAT_LAUNCH_CHECK();
  return 0;
}
