// goat_attn_long_fwd / goat_attn_long_bwd: masked multi-head attention (head_dim 64) for up to 512 keys (RxR-length instructions).
//
// attention.hip's forward keeps the whole score row-block of a 32-query tile in accumulators (f32x16 s[NKT], NKT <= 8); sixteen
// key tiles would be 256 accumulator VGPRs per wave.  Here the keys are streamed instead: a block of four waves (four 32-query
// tiles of one (sample, head)) walks the keys 32 at a time; each K|V tile is staged once in LDS for the four waves, the loads of
// tile j+1 are in flight (in registers) while tile j's MFMAs run, and every wave keeps a running row maximum m, row sum l and the
// rescaled output accumulators (the online softmax).  The score tile stays transposed as in attention.hip (S^T = K·Q^T: keys in
// the accumulator rows, the lane's query across lanes), and so does the output (O^T = V^T·P^T: head columns in the accumulator
// rows), so m, l and the rescale factor are lane-local apart from one cross-half shuffle per tile.
// Dropout draws AttnMask<T>::keep, the decision of the other two families.  The backward pass is attention.hip's dQ / dK|dV pair,
// whose register arrays do not depend on the length (512 K rows in LDS: 72 KiB bf16, 136 KiB f32).
#include "attn_tile.hpp"

namespace {

constexpr int LONG_MAXLK = 512;
constexpr int LONG_WAVES = 4;                      // 32-query tiles per block

template <typename T> struct Stage {               // this thread's share of one K|V tile: 2 * 32 rows of 64 / NE chunks over 256 threads
  static constexpr int CPR = HD / AT<T>::NE;       // 16-byte chunks per row
  static constexpr int N = 2 * 32 * CPR / (64 * LONG_WAVES);   // bf16 2, f32 4
  uint4 v[N];
  // chunk i of thread tid: tensor (K, V), row and chunk-in-row
  static __device__ __forceinline__ void where(int i, int tid, int& kv, int& r, int& cc) {
    const int c = i * 64 * LONG_WAVES + tid;
    kv = c / (32 * CPR);
    r = (c / CPR) % 32;
    cc = c % CPR;
  }
  __device__ __forceinline__ void load(const T* Kb, int64_t k_rs, const T* Vb, int64_t v_rs, int key0, int Lk, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int kv, r, cc;
      where(i, tid, kv, r, cc);
      uint4 x = {0u, 0u, 0u, 0u};                  // rows past Lk: zeros (their scores are set to -inf below, their V rows multiply 0)
      if (key0 + r < Lk) {
        const T* row = kv ? Vb + (int64_t)(key0 + r) * v_rs : Kb + (int64_t)(key0 + r) * k_rs;
        x = *reinterpret_cast<const uint4*>(row + cc * AT<T>::NE);
      }
      v[i] = x;
    }
  }
  __device__ __forceinline__ void store(T* kl, T* vl, int tid) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int kv, r, cc;
      where(i, tid, kv, r, cc);
      *reinterpret_cast<uint4*>((kv ? vl : kl) + r * AT<T>::LSTR + cc * AT<T>::NE) = v[i];
    }
  }
};

template <typename T>
__global__ __launch_bounds__(64 * LONG_WAVES) void attn_long_fwd_kernel(AttnArgs p) {
  typedef typename AT<T>::Frag Frag;
  constexpr int KSTEPS = AT<T>::KSTEPS, LSTR = AT<T>::LSTR, TSTEPS = AT<T>::TSTEPS, NE = AT<T>::NE;
  __shared__ __attribute__((aligned(16))) T kls[2][32 * LSTR];     // two K tiles and two V tiles: 18 KiB bf16, 34 KiB f32
  __shared__ __attribute__((aligned(16))) T vls[2][32 * LSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / p.nh, h = blockIdx.x % p.nh;
  const int q0 = (blockIdx.y * LONG_WAVES + wave) * 32;
  const int nkt = (p.Lk + 31) / 32;

  const T* Qb = reinterpret_cast<const T*>(p.Q) + b * p.q_bs + h * HD;
  const T* Kb = reinterpret_cast<const T*>(p.K) + b * p.k_bs + h * HD;
  const T* Vb = reinterpret_cast<const T*>(p.V) + b * p.v_bs + h * HD;
  T* Ob = reinterpret_cast<T*>(p.Ow) + b * p.o_bs + h * HD;

  Stage<T> stg;
  stg.load(Kb, p.k_rs, Vb, p.v_rs, 0, p.Lk, tid);

  const int q = q0 + l31;
  const bool qv = q < p.Lq;         // (a wave whose tile lies past Lq only stages and meets the barriers)
  Frag qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = gfrag<T>(Qb + (int64_t)q * p.q_rs, qv, ks, hi);

  const bool drop = p.p > 0.f;
  const uint32_t thr = goat_thr16(p.p);
  const float keep_scale = drop ? 1.f / (1.f - p.p) : 1.f;
  const AttnMask<T> rng(p, b, h);
  const float* kmask = p.kmask ? p.kmask + (int64_t)b * p.Lk : nullptr;
  const float* bias = (p.bias && qv) ? p.bias + ((int64_t)b * p.Lq + q) * p.Lk : nullptr;

  // O^T tiles: rows = head columns dt*32 + c_row(r) (accumulator regs), cols = queries (lanes)
  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -INFINITY;              // running maximum of the lane's query row (both halves agree)
  float l = 0.f;                    // running sum over the keys THIS half-wave holds; the halves are added once at the end

  stg.store(kls[0], vls[0], tid);
  __syncthreads();

  for (int jt = 0; jt < nkt; ++jt) {
    const T* kl = kls[jt & 1];
    const T* vl = vls[jt & 1];
    if (jt + 1 < nkt) stg.load(Kb, p.k_rs, Vb, p.v_rs, (jt + 1) * 32, p.Lk, tid);   // in flight during this tile's MFMAs

    if (q0 < p.Lq) {                // (wave-uniform)
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        Frag kf = *reinterpret_cast<const Frag*>(kl + l31 * LSTR + (ks * 2 + hi) * NE);
        mma32(s, kf, qf[ks]);
      }
      float mt = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = jt * 32 + c_row(r, lane);
        float v = -INFINITY;
        if (key < p.Lk) {
          v = s[r] * p.scale;
          if (kmask) v += kmask[key];
          if (bias) v += bias[key];
        }
        s[r] = v;
        mt = fmaxf(mt, v);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mn = fmaxf(m, mt);
      // every key so far at -inf: mn = -inf; subtract 0 instead, so that e = exp(-inf) = 0 and alpha = exp(-inf) = 0 (never inf - inf)
      const float msafe = (mn == -INFINITY) ? 0.f : mn;
      const float alpha = __expf(m - msafe);
      m = mn;
      float lt = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float e = __expf(s[r] - msafe);
        lt += e;
        if (drop) {
          const int key = jt * 32 + c_row(r, lane);
          e = rng.keep(p, q, key, thr) ? e * keep_scale : 0.f;
        }
        s[r] = e;
      }
      l = l * alpha + lt;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
      // O^T (d x q) += V^T (d x keys) · P^T (keys x q): V^T rows gathered from the row-major tile, P^T straight from the accumulators
#pragma unroll
      for (int st = 0; st < TSTEPS; ++st) {
        Frag pb = acc_frag<T>(s, st);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          Frag va = bfrag_crow<T>(vl, LSTR, 0, st, dt, lane);
          mma32(o[dt], va, pb);
        }
      }
    }
    if (jt + 1 < nkt) stg.store(kls[(jt + 1) & 1], vls[(jt + 1) & 1], tid);   // last read before the barrier that ended tile jt - 1
    __syncthreads();
  }

  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (!qv) return;
  if (hi == 0) p.lse[((int64_t)b * p.nh + h) * p.Lq + q] = (l > 0.f) ? (m + __logf(l)) : -INFINITY;
  // lane (q, hi) holds head columns dt*32 + 8*g + 4*hi + {0..3}, g < 4: four consecutive elements per store
  T* orow = Ob + (int64_t)q * p.o_rs;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      typedef T quad __attribute__((ext_vector_type(4)));
      quad w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = from_f<T>(o[dt][g * 4 + e] * inv);
      *reinterpret_cast<quad*>(orow + dt * 32 + 8 * g + 4 * hi) = w;
    }
}

template <typename T>
int launch_long_fwd(hipStream_t st, const AttnArgs& a) {
  const int nqt = (a.Lq + 31) / 32;
  hipLaunchKernelGGL(attn_long_fwd_kernel<T>, dim3(a.B * a.nh, (nqt + LONG_WAVES - 1) / LONG_WAVES), dim3(64 * LONG_WAVES), 0, st, a);
  GOAT_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int goat_attn_long_fwd(void* stream, int dtype, const void* Q, int64_t q_rs, int64_t q_bs, const void* K,
                                  int64_t k_rs, int64_t k_bs, const void* V, int64_t v_rs, int64_t v_bs, void* O,
                                  int64_t o_rs, int64_t o_bs, const float* kmask, const float* bias, float* lse, int B,
                                  int nh, int Lq, int Lk, float scale, float p, uint64_t seed, uint64_t offset,
                                  const uint64_t* rng_dev) {
  AttnArgs a;
  if (int e = attn_fwd_args(a, LONG_MAXLK, true, dtype, Q, q_rs, q_bs, K, k_rs, k_bs, V, v_rs, v_bs, O, o_rs, o_bs, kmask, bias, lse, B,
                            nh, Lq, Lk, scale, p, seed, offset, rng_dev))
    return e;
  return dtype_dispatch(dtype, [&](auto dt) -> int { return launch_long_fwd<GOAT_DT_TYPE(dt)>(ST(stream), a); });
}

extern "C" int goat_attn_long_bwd(void* stream, int dtype, const void* Q, int64_t q_rs, int64_t q_bs, const void* K,
                                  int64_t k_rs, int64_t k_bs, const void* V, int64_t v_rs, int64_t v_bs, const void* O,
                                  int64_t o_rs, int64_t o_bs, const void* dO, int64_t do_rs, int64_t do_bs, void* dQ,
                                  int64_t dq_rs, int64_t dq_bs, void* dK, int64_t dk_rs, int64_t dk_bs, void* dV,
                                  int64_t dv_rs, int64_t dv_bs, const float* kmask, const float* bias, const float* lse,
                                  float* dbias, int B, int nh, int Lq, int Lk, float scale, float p, uint64_t seed,
                                  uint64_t offset, const uint64_t* rng_dev) {
  AttnArgs a;
  if (int e = attn_bwd_args(a, LONG_MAXLK, dtype, Q, q_rs, q_bs, K, k_rs, k_bs, V, v_rs, v_bs, O, o_rs, o_bs, dO, do_rs, do_bs, dQ, dq_rs,
                            dq_bs, dK, dk_rs, dk_bs, dV, dv_rs, dv_bs, kmask, bias, lse, dbias, B, nh, Lq, Lk, scale, p, seed, offset,
                            rng_dev))
    return e;
  return goat_attn_tile_bwd(ST(stream), a, dtype);
}
