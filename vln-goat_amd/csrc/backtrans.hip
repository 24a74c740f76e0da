// goat_retok_rows / goat_scale_cols: the two device pieces of the back-translation augmentation (M/r2r/agent.py:457-474) around the
// speaker's decode loop — the decoded words become the agent's instruction without leaving the device, and one environment-dropout
// mask is multiplied into feature columns.
//
// goat_retok_rows — one block of four waves per row of decoded words; integers only.  Thread i owns columns 2i and 2i + 1 of the row
// (and later kept words 2i and 2i + 1), so that a block prefix sum over one count per thread keeps the order of the row:
//   1. the row goes to LDS as int32 (a word outside [0, V) is a status, not a read past the tables);
//   2. `shrink` (M/utils/data.py:373-398): column i < width - 1 is kept where w[i] != w[i + 1]; an exclusive block scan of the keep flags
//      compacts the kept words in LDS;
//   3. the first <EOS> and the first <PAD> of the kept list are block minimum reductions; start / end follow the reference's rules;
//   4. every sentence word looks up its id count in the CSR table of its place (sentence-initial or not); a second exclusive scan gives
//      the offset of its ids in the output row, and the thread that owns the word copies them, cut at max_len;
//   5. [agent_bos] at slot 0, [agent_eos] behind the ids if it still fits, fill_id and a zero mask byte behind the row's length.
// No thread writes a slot another thread writes, and nothing is atomic.  With width == 0 every block derives the width from the decode
// state itself (a maximum over at most 1024 end steps): no launch in front of this one, no host read.
//
// goat_scale_cols — out[r, c] = x[r, c] * noise[c] for c < D over rows of leading dimension ld: a grid-stride loop over 16-byte chunks
// when bases, ld and the noise vector allow it (a chunk then never straddles two rows; one that straddles column D is handled per
// element), over single elements otherwise.  One float32 multiply, rounded once to the storage type.
#include "common.hpp"

namespace {

constexpr int RT_MAXL = 512;          // DECODE_MAXL of the decode kernels: columns of a row of words
constexpr int RT_MAXB = 1024;
constexpr int RT_THREADS = 256;
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_NONE = 1 << 30;

// max / min of one int per thread over the block; every thread gets the result
template <bool MAX>
__device__ __forceinline__ int block_reduce_int(int v, int* buf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = MAX ? max(v, t) : min(v, t);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) buf[wave] = v;
  __syncthreads();
  int r = buf[0];
#pragma unroll
  for (int w = 1; w < RT_WAVES; ++w) r = MAX ? max(r, buf[w]) : min(r, buf[w]);
  return r;
}

// exclusive prefix sum of one int per thread in thread order; total = the sum over the block
__device__ __forceinline__ int block_scan_excl(int v, int* buf, int& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) buf[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < RT_WAVES; ++w) {
    if (w < wave) base += buf[w];
    tot += buf[w];
  }
  total = tot;
  return base + inc - v;
}

struct RetokArgs {
  const int64_t* words;
  int64_t ldw;
  const uint8_t* ended;
  const int32_t *end_step, *pos, *n_live;
  int width, B, V, bos, eos, pad;
  const int32_t *first_start, *first_ids, *rest_start, *rest_ids;
  int agent_bos, agent_eos, max_len;
  int64_t fill_id;
  int64_t* out_ids;
  uint8_t* out_mask;
  int64_t ldo;
  int32_t *lens, *status;
};

__global__ __launch_bounds__(RT_THREADS) void retok_rows_kernel(RetokArgs a) {
  __shared__ int w[RT_MAXL];          // the row
  __shared__ int kw[RT_MAXL];         // the words `shrink` keeps
  __shared__ int buf[RT_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;

  int width = a.width;
  if (width == 0) {                   // as infer_batch_cached cuts its result
    int m = -1;
    for (int r = tid; r < a.B; r += RT_THREADS)
      if (a.ended[r]) m = max(m, a.end_step[r]);
    m = block_reduce_int<true>(m, buf);
    width = *a.n_live > 0 ? *a.pos + 1 : m + 2;
  }
  // (st is block-uniform: every branch on it is taken by the whole block)
  int st = (width < 2 || width > a.ldw) ? GOAT_RETOK_E_WIDTH : 0;

  if (!st) {
    const int64_t* row = a.words + (int64_t)b * a.ldw;
    int bad = 0;
    for (int c = tid; c < width; c += RT_THREADS) {
      const int64_t v = row[c];
      if (v < 0 || v >= a.V) bad = 1;
      w[c] = bad ? 0 : (int)v;
    }
    if (block_reduce_int<true>(bad, buf)) st = GOAT_RETOK_E_WORD;      // (its barriers publish w)
  }

  int n_out = 0;
  if (!st) {
    const int c0 = 2 * tid, c1 = c0 + 1;
    const int k0 = (c0 < width - 1 && w[c0] != w[c0 + 1]) ? 1 : 0;
    const int k1 = (c1 < width - 1 && w[c1] != w[c1 + 1]) ? 1 : 0;
    int len;
    const int at = block_scan_excl(k0 + k1, buf, len);
    if (k0) kw[at] = w[c0];
    if (k1) kw[at + k0] = w[c1];
    __syncthreads();
    if (len == 0) st = GOAT_RETOK_E_EMPTY;      // one run over the whole row: np.argmax of an empty list raises in the reference
    if (!st) {
      // kept words c0, c1 are this thread's from here on
      int e = RT_NONE;
      if (c1 < len && kw[c1] == a.eos) e = c1;
      if (c0 < len && kw[c0] == a.eos) e = c0;
      int end = block_reduce_int<false>(e, buf);
      if (end == RT_NONE || end == 0) end = len;            // np.argmax(...) == 0: no <EOS>, or <EOS> first
      const int start = (len > 1 && kw[0] == a.bos) ? 1 : 0;
      e = RT_NONE;
      if (c1 >= start && c1 < end && kw[c1] == a.pad) e = c1;
      if (c0 >= start && c0 < end && kw[c0] == a.pad) e = c0;
      const int send = min(end, block_reduce_int<false>(e, buf));      // decode_sentence stops at the first <PAD>

      int s0 = 0, n0 = 0, s1 = 0, n1 = 0;
      const int32_t *i0 = nullptr, *i1 = nullptr;
      if (c0 >= start && c0 < send) {
        const bool first = c0 == start;
        const int32_t* ts = first ? a.first_start : a.rest_start;
        i0 = first ? a.first_ids : a.rest_ids;
        s0 = ts[kw[c0]];
        n0 = min(max(ts[kw[c0] + 1] - s0, 0), a.max_len);   // (more than max_len ids are cut anyway: the sums stay small)
      }
      if (c1 >= start && c1 < send) {
        const bool first = c1 == start;
        const int32_t* ts = first ? a.first_start : a.rest_start;
        i1 = first ? a.first_ids : a.rest_ids;
        s1 = ts[kw[c1]];
        n1 = min(max(ts[kw[c1] + 1] - s1, 0), a.max_len);
      }
      int total;
      const int off = block_scan_excl(n0 + n1, buf, total);
      int64_t* out = a.out_ids + (int64_t)b * a.ldo;
      int p = 1 + off;
      for (int j = 0; j < n0 && p + j < a.max_len; ++j) out[p + j] = (int64_t)i0[s0 + j];
      p += n0;
      for (int j = 0; j < n1 && p + j < a.max_len; ++j) out[p + j] = (int64_t)i1[s1 + j];
      if (tid == 0) {
        out[0] = (int64_t)a.agent_bos;
        if (1 + total < a.max_len) out[1 + total] = (int64_t)a.agent_eos;      // a plain slice: a long sentence loses its </s>
      }
      n_out = min(a.max_len, total + 2);
    }
  }

  int64_t* out = a.out_ids + (int64_t)b * a.ldo;
  uint8_t* mask = a.out_mask + (int64_t)b * a.ldo;
  for (int64_t j = tid; j < a.ldo; j += RT_THREADS) {
    if (j >= n_out) out[j] = a.fill_id;
    mask[j] = j < n_out ? 1 : 0;
  }
  if (tid == 0) {
    a.lens[b] = n_out;
    a.status[b] = st;
  }
}

// ------------------------------------------------------------------------------------------------ goat_scale_cols
constexpr int SC_THREADS = 256;
constexpr int SC_MAXBLOCKS = 2048;

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void scale_cols_vec_kernel(const T* x, T* out, const float* noise, int64_t rows, int64_t ld, int D) {
  constexpr int NE = DT<T>::EPC;
  const int64_t cpr = ld / NE, n = rows * cpr;
  const bool inplace = x == out;
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SC_THREADS) {
    const int c = (int)(i % cpr) * NE;
    if (c >= D && inplace) continue;
    const int64_t at = (i / cpr) * ld + c;
    Chunk<T> ch;
    ch.load(x + at);
    if (c + NE <= D) {
#pragma unroll
      for (int q = 0; q < NE / 4; ++q) {
        const f32x4 nz = *reinterpret_cast<const f32x4*>(noise + c + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) ch.v[4 * q + e] *= nz[e];
      }
    } else if (c < D) {
#pragma unroll
      for (int e = 0; e < NE; ++e)
        if (c + e < D) ch.v[e] *= noise[c + e];
    }
    ch.store(out + at);               // (a bf16 value that was only widened converts back to itself: the copy is exact)
  }
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void scale_cols_scalar_kernel(const T* x, T* out, const float* noise, int64_t rows, int64_t ld, int D) {
  const int64_t n = rows * ld;
  const bool inplace = x == out;
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SC_THREADS) {
    const int c = (int)(i % ld);
    if (c < D) out[i] = from_f<T>(to_f(x[i]) * noise[c]);
    else if (!inplace) out[i] = x[i];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int goat_retok_rows(void* stream, const int64_t* words, int64_t ldw, const uint8_t* ended, const int32_t* end_step,
                               const int32_t* pos_dev, const int32_t* n_live, int width, int B, int V, int bos, int eos, int pad,
                               const int32_t* first_start, const int32_t* first_ids, const int32_t* rest_start, const int32_t* rest_ids,
                               int agent_bos, int agent_eos, int64_t fill_id, int max_len, int64_t* out_ids, uint8_t* out_mask,
                               int64_t ldo, int32_t* lens, int32_t* status) {
  if (!words || !first_start || !first_ids || !rest_start || !rest_ids || !out_ids || !out_mask || !lens || !status) return GOAT_E_ARG;
  if (width == 0 && (!ended || !end_step || !pos_dev || !n_live)) return GOAT_E_ARG;
  if (ldw < 1 || ldw > RT_MAXL || width < 0 || width > RT_MAXL) return GOAT_E_SHAPE;
  if (max_len < 2 || max_len > RT_MAXL || max_len > ldo) return GOAT_E_SHAPE;
  if (B < 1 || B > RT_MAXB || V < 1) return GOAT_E_SHAPE;
  RetokArgs a = {};
  a.words = words; a.ldw = ldw; a.ended = ended; a.end_step = end_step; a.pos = pos_dev; a.n_live = n_live;
  a.width = width; a.B = B; a.V = V; a.bos = bos; a.eos = eos; a.pad = pad;
  a.first_start = first_start; a.first_ids = first_ids; a.rest_start = rest_start; a.rest_ids = rest_ids;
  a.agent_bos = agent_bos; a.agent_eos = agent_eos; a.max_len = max_len; a.fill_id = fill_id;
  a.out_ids = out_ids; a.out_mask = out_mask; a.ldo = ldo; a.lens = lens; a.status = status;
  hipLaunchKernelGGL(retok_rows_kernel, dim3(B), dim3(RT_THREADS), 0, ST(stream), a);
  GOAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int goat_scale_cols(void* stream, int dtype, const void* x, void* out, const float* noise, int64_t rows, int64_t ld, int D) {
  if (!x || !out || !noise) return GOAT_E_ARG;
  if (rows < 1 || D < 1 || ld < D || rows > INT64_MAX / ld) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    constexpr int NE = DT<T>::EPC;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) % sizeof(T)) return GOAT_E_SHAPE;
    const bool vec = aligned16(x) && aligned16(out) && aligned16(noise) && ld % NE == 0;
    const int64_t n = vec ? rows * (ld / NE) : rows * ld;
    int64_t blocks = (n + SC_THREADS - 1) / SC_THREADS;
    if (blocks > SC_MAXBLOCKS) blocks = SC_MAXBLOCKS;
    if (vec)
      hipLaunchKernelGGL(scale_cols_vec_kernel<T>, dim3((unsigned)blocks), dim3(SC_THREADS), 0, ST(stream), reinterpret_cast<const T*>(x),
                         reinterpret_cast<T*>(out), noise, rows, ld, D);
    else
      hipLaunchKernelGGL(scale_cols_scalar_kernel<T>, dim3((unsigned)blocks), dim3(SC_THREADS), 0, ST(stream), reinterpret_cast<const T*>(x),
                         reinterpret_cast<T*>(out), noise, rows, ld, D);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}
