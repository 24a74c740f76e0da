// goat_attn_fwd / goat_attn_bwd: masked multi-head attention (head_dim 64) on MFMA 32x32 tiles.
//
// GOAT's sequences are tiny (36 views, <=80..200 tokens, <=~60 map nodes), so instead of flash-style
// streaming one workgroup owns a whole (sample, head): forward = one wave per 32-query tile with the full
// score row-block held in accumulators (S^T = K·Q^T, so a softmax row is lane-local: keys live in the
// accumulator registers, queries across lanes); V (forward) / K, Q_i, dO_i (backward) are staged row-major
// in LDS and the "transposed" MFMA operands are gathered from there, exploiting that the k-order inside an
// MFMA step is free as long as A and B agree.  Dropout on the probabilities uses the stateless counter hash
// of common.hpp and is regenerated in the backward pass.
#include <cstdlib>
#include "attn_tile.hpp"

namespace {

// ======================================================================================== forward
template <typename T, int NKT>
__global__ __launch_bounds__(512) void attn_fwd_kernel(AttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename AT<T>::Frag Frag;
  constexpr int KSTEPS = AT<T>::KSTEPS, LSTR = AT<T>::LSTR, TSTEPS = AT<T>::TSTEPS;
  T* vl = reinterpret_cast<T*>(smem);  // [NKT*32][LSTR]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / p.nh, h = blockIdx.x % p.nh;
  const int q0 = (blockIdx.y * (blockDim.x >> 6) + wave) * 32;

  const T* Qb = reinterpret_cast<const T*>(p.Q) + b * p.q_bs + h * HD;
  const T* Kb = reinterpret_cast<const T*>(p.K) + b * p.k_bs + h * HD;
  const T* Vb = reinterpret_cast<const T*>(p.V) + b * p.v_bs + h * HD;
  T* Ob = reinterpret_cast<T*>(p.Ow) + b * p.o_bs + h * HD;

  stage_rows<T>(vl, Vb, p.v_rs, 0, p.Lk, NKT * 32, tid, blockDim.x);

  const int q = q0 + l31;
  const bool qv = q < p.Lq;
  Frag qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = gfrag<T>(Qb + (int64_t)q * p.q_rs, qv, ks, hi);

  // S^T tiles: rows = keys (accumulator regs), cols = queries (lanes)
  f32x16 s[NKT];
#pragma unroll
  for (int jt = 0; jt < NKT; ++jt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[jt][r] = 0.f;
    const int key = jt * 32 + l31;
    const bool kv = key < p.Lk;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      Frag kf = gfrag<T>(Kb + (int64_t)key * p.k_rs, kv, ks, hi);
      mma32(s[jt], kf, qf[ks]);
    }
  }

  // scale + masks, row max
  float m = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < NKT; ++jt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = jt * 32 + c_row(r, lane);
      float v = -INFINITY;
      if (key < p.Lk) {
        v = s[jt][r] * p.scale;
        if (p.kmask) v += p.kmask[(int64_t)b * p.Lk + key];
        if (p.bias && qv) v += p.bias[((int64_t)b * p.Lq + q) * p.Lk + key];
      }
      s[jt][r] = v;
      m = fmaxf(m, v);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l = 0.f;
  const float msafe = (m == -INFINITY) ? 0.f : m;
#pragma unroll
  for (int jt = 0; jt < NKT; ++jt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float e = __expf(s[jt][r] - msafe);
      s[jt][r] = e;
      l += e;
    }
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (qv && hi == 0) p.lse[((int64_t)b * p.nh + h) * p.Lq + q] = (l > 0.f) ? (msafe + __logf(l)) : -INFINITY;

  const bool drop = p.p > 0.f;
  const uint32_t thr = goat_thr16(p.p);
  const float keep_scale = drop ? 1.f / (1.f - p.p) : 1.f;
  const AttnMask<T> rng(p, b, h);
#pragma unroll
  for (int jt = 0; jt < NKT; ++jt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float pv = s[jt][r] * inv;
      if (drop) {
        const int key = jt * 32 + c_row(r, lane);
        pv = rng.keep(p, q, key, thr) ? pv * keep_scale : 0.f;
      }
      s[jt][r] = pv;
    }

  __syncthreads();  // V staged

  // O (q x d) = P (q x keys) · V (keys x d)
  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
  for (int jt = 0; jt < NKT; ++jt)
#pragma unroll
    for (int st = 0; st < TSTEPS; ++st) {
      Frag pa = acc_frag<T>(s[jt], st);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        Frag vb = bfrag_crow<T>(vl, LSTR, jt * 32, st, dt, lane);
        mma32(o[dt], pa, vb);
      }
    }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = q0 + c_row(r, lane);
      if (qq < p.Lq) Ob[(int64_t)qq * p.o_rs + dt * 32 + l31] = from_f<T>(o[dt][r]);
    }
}

// ======================================================================================== backward
// Two barrier-free single-wave roles per (b, h); S and dP are recomputed in each (cheaper than the cross-wave
// reductions, LDS transposes and barriers of a one-workgroup-per-head kernel: 17 % -> 8 % of the step):
//   dQ role  (b, h, q-tile):  lane = query;  S^T = K·Q^T, dP^T = V·dO^T per key tile; dQ += dS·K
//   dKV role (b, h, key-tile): lane = key;   S = Q·K^T, dP = dO·V^T per query tile; dV += Pd^T·dO, dK += dS^T·Q
// "Transposed" B operands (K, dO, Q with the contraction index as the LDS row) come from bfrag_crow.
template <typename T>
__global__ __launch_bounds__(64) void attn_bwd_dq_kernel(AttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename AT<T>::Frag Frag;
  constexpr int KSTEPS = AT<T>::KSTEPS, LSTR = AT<T>::LSTR, TSTEPS = AT<T>::TSTEPS, NE = AT<T>::NE;
  T* kl = reinterpret_cast<T*>(smem);  // [nkt*32][LSTR]
  const int lane = threadIdx.x, hi = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / p.nh, h = blockIdx.x % p.nh;
  const int q0 = blockIdx.y * 32, q = q0 + l31;
  const bool qv = q < p.Lq;
  const int nkt = (p.Lk + 31) / 32;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + b * p.q_bs + h * HD;
  const T* Kb = reinterpret_cast<const T*>(p.K) + b * p.k_bs + h * HD;
  const T* Vb = reinterpret_cast<const T*>(p.V) + b * p.v_bs + h * HD;
  const T* Ob = reinterpret_cast<const T*>(p.O) + b * p.o_bs + h * HD;
  const T* dOb = reinterpret_cast<const T*>(p.dO) + b * p.do_bs + h * HD;
  T* dQb = reinterpret_cast<T*>(p.dQ) + b * p.dq_bs + h * HD;

  stage_rows<T>(kl, Kb, p.k_rs, 0, p.Lk, nkt * 32, lane, 64);
  Frag qf[KSTEPS], dof[KSTEPS];
  float dsum = 0.f;
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    qf[ks] = gfrag<T>(Qb + (int64_t)q * p.q_rs, qv, ks, hi);
    dof[ks] = gfrag<T>(dOb + (int64_t)q * p.do_rs, qv, ks, hi);
    Frag of = gfrag<T>(Ob + (int64_t)q * p.o_rs, qv, ks, hi);
#pragma unroll
    for (int e = 0; e < NE; ++e) dsum += to_f(dof[ks][e]) * to_f(of[e]);
  }
  dsum += __shfl_xor(dsum, 32, 64);
  const float lse_q = qv ? p.lse[((int64_t)b * p.nh + h) * p.Lq + q] : 0.f;
  const bool lse_ok = (lse_q != -INFINITY);
  const bool drop = p.p > 0.f;
  const uint32_t thr = goat_thr16(p.p);
  const float keep_scale = drop ? 1.f / (1.f - p.p) : 1.f;
  const AttnMask<T> rng(p, b, h);
  __syncthreads();

  f32x16 dq[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
  for (int jt = 0; jt < nkt; ++jt) {
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
    const int key_l = jt * 32 + l31;
    const bool kvl = key_l < p.Lk;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      Frag kf = *reinterpret_cast<const Frag*>(kl + key_l * LSTR + (ks * 2 + hi) * NE);
      Frag vf = gfrag<T>(Vb + (int64_t)key_l * p.v_rs, kvl, ks, hi);
      mma32(s, kf, qf[ks]);
      mma32(dp, vf, dof[ks]);
    }
    f32x16 ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = jt * 32 + c_row(r, lane);
      float pr = 0.f;
      if (qv && key < p.Lk && lse_ok) {
        float v = s[r] * p.scale;
        if (p.kmask) v += p.kmask[(int64_t)b * p.Lk + key];
        if (p.bias) v += p.bias[((int64_t)b * p.Lq + q) * p.Lk + key];
        pr = __expf(v - lse_q);
      }
      float keep = 1.f;
      if (drop) keep = rng.keep(p, q, key, thr) ? keep_scale : 0.f;
      const float d = pr * (dp[r] * keep - dsum);
      if (p.dbias && qv && key < p.Lk) atomicAdd(p.dbias + ((int64_t)b * p.Lq + q) * p.Lk + key, d);
      ds[r] = d * p.scale;
    }
#pragma unroll
    for (int st = 0; st < TSTEPS; ++st) {
      Frag a = acc_frag<T>(ds, st);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        Frag kb = bfrag_crow<T>(kl, LSTR, jt * 32, st, dt, lane);
        mma32(dq[dt], a, kb);
      }
    }
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = q0 + c_row(r, lane);
      if (qq < p.Lq) dQb[(int64_t)qq * p.dq_rs + dt * 32 + l31] = from_f<T>(dq[dt][r]);
    }
}

template <typename T>
__global__ __launch_bounds__(64) void attn_bwd_dkv_kernel(AttnArgs p) {
  typedef typename AT<T>::Frag Frag;
  constexpr int KSTEPS = AT<T>::KSTEPS, LSTR = AT<T>::LSTR, TSTEPS = AT<T>::TSTEPS, NE = AT<T>::NE;
  __shared__ __attribute__((aligned(16))) T ql[32 * AT<T>::LSTR];
  __shared__ __attribute__((aligned(16))) T dol[32 * AT<T>::LSTR];
  __shared__ float rowd[32], rowl[32];
  const int lane = threadIdx.x, hi = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / p.nh, h = blockIdx.x % p.nh;
  const int k0 = blockIdx.y * 32, key = k0 + l31;
  const bool kv = key < p.Lk;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + b * p.q_bs + h * HD;
  const T* Kb = reinterpret_cast<const T*>(p.K) + b * p.k_bs + h * HD;
  const T* Vb = reinterpret_cast<const T*>(p.V) + b * p.v_bs + h * HD;
  const T* Ob = reinterpret_cast<const T*>(p.O) + b * p.o_bs + h * HD;
  const T* dOb = reinterpret_cast<const T*>(p.dO) + b * p.do_bs + h * HD;
  T* dKb = reinterpret_cast<T*>(p.dK) + b * p.dk_bs + h * HD;
  T* dVb = reinterpret_cast<T*>(p.dV) + b * p.dv_bs + h * HD;

  Frag kf[KSTEPS], vf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    kf[ks] = gfrag<T>(Kb + (int64_t)key * p.k_rs, kv, ks, hi);
    vf[ks] = gfrag<T>(Vb + (int64_t)key * p.v_rs, kv, ks, hi);
  }
  const float kmv = kv ? (p.kmask ? p.kmask[(int64_t)b * p.Lk + key] : 0.f) : -INFINITY;
  const bool drop = p.p > 0.f;
  const uint32_t thr = goat_thr16(p.p);
  const float keep_scale = drop ? 1.f / (1.f - p.p) : 1.f;
  const AttnMask<T> rng(p, b, h);

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }

  const int nqt = (p.Lq + 31) / 32;
  for (int it = 0; it < nqt; ++it) {
    const int q0 = it * 32;
    __syncthreads();
    stage_rows<T>(ql, Qb, p.q_rs, q0, p.Lq, 32, lane, 64);
    stage_rows<T>(dol, dOb, p.do_rs, q0, p.Lq, 32, lane, 64);
    {  // D_q and lse_q for row l31 of this query tile
      const int qq = q0 + l31;
      float dsum = 0.f;
      if (qq < p.Lq) {
        const T* orow = Ob + (int64_t)qq * p.o_rs + hi * 32;
        const T* drow = dOb + (int64_t)qq * p.do_rs + hi * 32;
#pragma unroll
        for (int c = 0; c < 32 / NE; ++c) {
          Chunk<T> a, d2;
          a.load(orow + c * NE);
          d2.load(drow + c * NE);
#pragma unroll
          for (int e = 0; e < NE; ++e) dsum += a.v[e] * d2.v[e];
        }
      }
      dsum += __shfl_xor(dsum, 32, 64);
      if (hi == 0) {
        rowd[l31] = dsum;
        rowl[l31] = (qq < p.Lq) ? p.lse[((int64_t)b * p.nh + h) * p.Lq + qq] : -INFINITY;
      }
    }
    __syncthreads();
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      Frag qa = *reinterpret_cast<const Frag*>(ql + l31 * LSTR + (ks * 2 + hi) * NE);
      Frag da = *reinterpret_cast<const Frag*>(dol + l31 * LSTR + (ks * 2 + hi) * NE);
      mma32(s, qa, kf[ks]);
      mma32(dp, da, vf[ks]);
    }
    f32x16 pd, ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = c_row(r, lane);
      const int q = q0 + qr;
      const float lse_q = rowl[qr];
      float pr = 0.f;
      if (q < p.Lq && kv && lse_q != -INFINITY) {
        float v = s[r] * p.scale + kmv;
        if (p.bias) v += p.bias[((int64_t)b * p.Lq + q) * p.Lk + key];
        pr = __expf(v - lse_q);
      }
      float keep = 1.f;
      if (drop) keep = rng.keep(p, q, key, thr) ? keep_scale : 0.f;
      pd[r] = pr * keep;
      ds[r] = pr * (dp[r] * keep - rowd[qr]) * p.scale;
    }
#pragma unroll
    for (int st = 0; st < TSTEPS; ++st) {
      Frag ap = acc_frag<T>(pd, st);
      Frag as = acc_frag<T>(ds, st);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        Frag bo = bfrag_crow<T>(dol, LSTR, 0, st, dt, lane);
        mma32(dv[dt], ap, bo);
        Frag bq = bfrag_crow<T>(ql, LSTR, 0, st, dt, lane);
        mma32(dk[dt], as, bq);
      }
    }
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = k0 + c_row(r, lane);
      if (kk < p.Lk) {
        dKb[(int64_t)kk * p.dk_rs + dt * 32 + l31] = from_f<T>(dk[dt][r]);
        dVb[(int64_t)kk * p.dv_rs + dt * 32 + l31] = from_f<T>(dv[dt][r]);
      }
    }
}

template <typename T>
int launch_bwd2(hipStream_t st, const AttnArgs& a) {
  const int nkt = (a.Lk + 31) / 32, nqt = (a.Lq + 31) / 32;
  const size_t sm = (size_t)nkt * 32 * AT<T>::LSTR * sizeof(T);
  if (int e = set_smem<attn_bwd_dq_kernel<T>>(sm)) return e;
  hipLaunchKernelGGL(attn_bwd_dq_kernel<T>, dim3(a.B * a.nh, nqt), dim3(64), sm, st, a);
  GOAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_bwd_dkv_kernel<T>, dim3(a.B * a.nh, nkt), dim3(64), 0, st, a);
  GOAT_LAUNCH_CHECK();
  return 0;
}

template <typename T>
size_t fwd_smem(int nkt) { return (size_t)nkt * 32 * AT<T>::LSTR * sizeof(T); }

template <typename T, int NKT>
int launch_fwd(hipStream_t st, const AttnArgs& a) {
  const int nqt = (a.Lq + 31) / 32;
  const int wpb = nqt < 8 ? nqt : 8;  // waves per block
  dim3 grid(a.B * a.nh, (nqt + wpb - 1) / wpb);
  size_t sm = fwd_smem<T>(NKT);
  if (int e = set_smem<attn_fwd_kernel<T, NKT>>(sm)) return e;
  hipLaunchKernelGGL((attn_fwd_kernel<T, NKT>), grid, dim3(64 * wpb), sm, st, a);
  GOAT_LAUNCH_CHECK();
  return 0;
}
template <typename T>
int dispatch_fwd(hipStream_t st, const AttnArgs& a) {
  const int nkt = (a.Lk + 31) / 32;
#define GOAT_ATTN_CASE(N) \
  case N: return launch_fwd<T, N>(st, a);
  switch (nkt) {
    GOAT_ATTN_CASE(1) GOAT_ATTN_CASE(2) GOAT_ATTN_CASE(3) GOAT_ATTN_CASE(4)
    GOAT_ATTN_CASE(5) GOAT_ATTN_CASE(6) GOAT_ATTN_CASE(7) GOAT_ATTN_CASE(8)
  }
#undef GOAT_ATTN_CASE
  return GOAT_E_SHAPE;
}

bool use_v2() {       // GOAT_ATTN_V1=1: the round-1 kernels for every problem (A/B experiments)
  static const bool v = !(getenv("GOAT_ATTN_V1") && getenv("GOAT_ATTN_V1")[0] == '1');
  return v;
}

}  // namespace

int goat_attn_tile_bwd(hipStream_t st, const AttnArgs& a, int dtype) {
  return dtype_dispatch(dtype, [&](auto dt) -> int { return launch_bwd2<GOAT_DT_TYPE(dt)>(st, a); });
}

extern "C" int goat_attn_fwd(void* stream, int dtype, const void* Q, int64_t q_rs, int64_t q_bs, const void* K,
                             int64_t k_rs, int64_t k_bs, const void* V, int64_t v_rs, int64_t v_bs, void* O,
                             int64_t o_rs, int64_t o_bs, const float* kmask, const float* bias, float* lse, int B,
                             int nh, int Lq, int Lk, float scale, float p, uint64_t seed, uint64_t offset,
                             const uint64_t* rng_dev) {
  AttnArgs a;
  if (int e = attn_fwd_args(a, 256, false, dtype, Q, q_rs, q_bs, K, k_rs, k_bs, V, v_rs, v_bs, O, o_rs, o_bs, kmask, bias, lse, B, nh, Lq,
                            Lk, scale, p, seed, offset, rng_dev))
    return e;
  if (dtype == GOAT_BF16 && use_v2()) {          // LDS-staged kernels (attention2.hip) first: GOAT_E_SHAPE means "not theirs"
    const int rc = goat_attn2_fwd(ST(stream), a);
    if (rc != GOAT_E_SHAPE) return rc;
  }
  return dtype_dispatch(dtype, [&](auto dt) -> int { return dispatch_fwd<GOAT_DT_TYPE(dt)>(ST(stream), a); });
}

extern "C" int goat_attn_bwd(void* stream, int dtype, const void* Q, int64_t q_rs, int64_t q_bs, const void* K,
                             int64_t k_rs, int64_t k_bs, const void* V, int64_t v_rs, int64_t v_bs, const void* O,
                             int64_t o_rs, int64_t o_bs, const void* dO, int64_t do_rs, int64_t do_bs, void* dQ,
                             int64_t dq_rs, int64_t dq_bs, void* dK, int64_t dk_rs, int64_t dk_bs, void* dV,
                             int64_t dv_rs, int64_t dv_bs, const float* kmask, const float* bias, const float* lse,
                             float* dbias, int B, int nh, int Lq, int Lk, float scale, float p, uint64_t seed,
                             uint64_t offset, const uint64_t* rng_dev) {
  AttnArgs a;
  if (int e = attn_bwd_args(a, 256, dtype, Q, q_rs, q_bs, K, k_rs, k_bs, V, v_rs, v_bs, O, o_rs, o_bs, dO, do_rs, do_bs, dQ, dq_rs, dq_bs,
                            dK, dk_rs, dk_bs, dV, dv_rs, dv_bs, kmask, bias, lse, dbias, B, nh, Lq, Lk, scale, p, seed, offset, rng_dev))
    return e;
  if (dtype == GOAT_BF16 && use_v2()) {
    const int rc = goat_attn2_bwd(ST(stream), a);
    if (rc != GOAT_E_SHAPE) return rc;
  }
  return goat_attn_tile_bwd(ST(stream), a, dtype);
}
