// Device-side tile helpers shared by the three attention families (attention.hip: one wave per tile, Lk <= 256, whole score row-block
// in accumulators; attention_long.hip: key-streaming forward for Lk <= 512; attention2.hip: the LDS-staged bf16 kernels): the tile
// constants AT<T>, fragment loads / gathers for MFMA 32x32 tiles of 64-wide head rows (bfrag_crow, acc_frag: all three families),
// and, for the two one-wave-per-tile families, the row staging copy and the dropout decision AttnMask (which draws attention2.hip's
// HeadRng bits for bf16).  The argument block, its builders and the other host helpers are in attn_args.hpp.
#pragma once
#include "attn_args.hpp"

namespace {

constexpr int HD = 64;  // head dim

template <typename T> struct AT {
  typedef typename FragT<T>::type Frag;
  static constexpr int NE = DT<T>::EPC;                 // elements per 16-B chunk
  static constexpr int ROWB = HD * (int)sizeof(T);      // bytes per head row
  static constexpr int KSTEPS = ROWB / 32;              // 32-byte k-steps over d (bf16 4, f32 8)
  static constexpr int LSTR = HD + NE;                  // LDS row stride (elements) of [row][64] tiles
  static constexpr int TSTEPS = 32 / (2 * NE);          // k-steps over a 32-wide tile (bf16 2, f32 4)
  static constexpr int PSTR = 32 + NE;                  // LDS row stride of [32][32] tiles
};

template <typename T>
__device__ __forceinline__ typename AT<T>::Frag zero_frag() {
  typename AT<T>::Frag f;
#pragma unroll
  for (int e = 0; e < AT<T>::NE; ++e) f[e] = (T)0.f;
  return f;
}

// 16-B chunk (ks, hi) of a 64-wide row in global memory
template <typename T>
__device__ __forceinline__ typename AT<T>::Frag gfrag(const T* row_ptr, bool valid, int ks, int hi) {
  typedef typename AT<T>::Frag Frag;
  if (!valid) return zero_frag<T>();
  return *reinterpret_cast<const Frag*>(row_ptr + (ks * 2 + hi) * AT<T>::NE);
}

// gather an MFMA B fragment "fixed column, accumulator-pattern rows" from a row-major LDS tile
template <typename T>
__device__ __forceinline__ typename AT<T>::Frag gather_crow(const T* lds, int stride, int row_base, int step, int col,
                                                             int lane) {
  typename AT<T>::Frag f;
#pragma unroll
  for (int e = 0; e < AT<T>::NE; ++e) f[e] = lds[(row_base + c_row(step * AT<T>::NE + e, lane)) * stride + col];
  return f;
}
// gather "fixed column, rows (2*step+hi)*NE + e"
template <typename T>
__device__ __forceinline__ typename AT<T>::Frag gather_lin(const T* lds, int stride, int step, int hi, int col) {
  typename AT<T>::Frag f;
#pragma unroll
  for (int e = 0; e < AT<T>::NE; ++e) f[e] = lds[((2 * step + hi) * AT<T>::NE + e) * stride + col];
  return f;
}
template <typename T>
__device__ __forceinline__ typename AT<T>::Frag acc_frag(const f32x16& a, int step) {
  typename AT<T>::Frag f;
#pragma unroll
  for (int e = 0; e < AT<T>::NE; ++e) f[e] = from_f<T>(a[step * AT<T>::NE + e]);
  return f;
}

// B fragment "fixed column, accumulator-pattern rows" of a row-major [row][64] LDS tile.
//   f32 : four ds_read_b32 (rows 8*step + 4*hi + e)
//   bf16: two ds_read_b64_tr_b16 (hardware 4x16 transpose): rows 16*step + 4*hi + {0..3} and +8
template <typename T>
__device__ __forceinline__ typename AT<T>::Frag bfrag_crow(const T* lds, int stride, int row_base, int step, int dt, int lane);
template <>
__device__ __forceinline__ f32x4 bfrag_crow<float>(const float* lds, int stride, int row_base, int step, int dt, int lane) {
  return gather_crow<float>(lds, stride, row_base, step, dt * 32 + (lane & 31), lane);
}
template <>
__device__ __forceinline__ bf16x8 bfrag_crow<bf16_t>(const bf16_t* lds, int stride, int row_base, int step, int dt, int lane) {
  typedef __attribute__((address_space(3))) bf16x4 lds_b4;
  const int g = lane >> 4, t15 = lane & 15;
  const int col = dt * 32 + (g & 1) * 16 + (t15 & 3) * 4;
  const int r0 = row_base + 16 * step + 4 * (g >> 1) + (t15 >> 2);
  bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(lds + r0 * stride + col));
  bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(lds + (r0 + 8) * stride + col));
  bf16x8 f;
  f[0] = v0[0]; f[1] = v0[1]; f[2] = v0[2]; f[3] = v0[3];
  f[4] = v1[0]; f[5] = v1[1]; f[6] = v1[2]; f[7] = v1[3];
  return f;
}

// cooperative copy of `nrows` 64-wide rows (global, strided) into LDS [rows_pad][LSTR]; rows >= nrows zero
template <typename T>
__device__ __forceinline__ void stage_rows(T* lds, const T* g, int64_t rs, int row0, int nrows_valid, int rows_pad,
                                           int tid, int nthreads) {
  constexpr int CPR = HD / AT<T>::NE;  // chunks per row
  for (int c = tid; c < rows_pad * CPR; c += nthreads) {
    int r = c / CPR, cc = c % CPR;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row0 + r < nrows_valid) v = *reinterpret_cast<const uint4*>(g + (int64_t)(row0 + r) * rs + cc * AT<T>::NE);
    *reinterpret_cast<uint4*>(lds + r * AT<T>::LSTR + cc * AT<T>::NE) = v;
  }
}

// Dropout decision for probability (b, h, q, key).  bf16: the per-head 32-bit hash of the LDS-staged kernels (attention2.hip's
// HeadRng) — goat_attn_fwd and goat_attn_bwd may be served by different kernel families for one call (the staged backward needs
// more LDS than the staged forward), so both families must draw the same bits.  f32 (always these kernels): the 64-bit counter
// stream of GoatRng, as documented in the header.
template <typename T>
struct AttnMask {
  GoatRng g;
  HeadRng hr;
  uint64_t base;
  __device__ __forceinline__ AttnMask(const AttnArgs& p, int b, int h)
      : g(p.seed + (p.rng_dev ? *p.rng_dev : 0ull)),
        hr(p.seed + (p.rng_dev ? *p.rng_dev : 0ull), p.offset, (uint32_t)(b * p.nh + h)),
        base(p.offset + ((uint64_t)b * p.nh + h) * (uint64_t)p.Lq * (uint64_t)p.Lk) {}
  __device__ __forceinline__ bool keep(const AttnArgs& p, int q, int key, uint32_t thr) const {
    if (sizeof(T) == 2) return hr.keep((uint32_t)q * (uint32_t)p.Lk + (uint32_t)key, thr);
    return g.keep(base + (uint64_t)q * (uint64_t)p.Lk + key, thr);
  }
};

}  // namespace
