// Host side shared by the three attention families (attention.hip: one wave per tile, any dtype, Lk <= 256; attention2.hip: the
// LDS-staged bf16 kernels for sequences of up to 256 rows; attention_long.hip: the key-streaming forward for Lk <= 512): the argument
// block the kernels take, the two builders that check and marshal the raw arguments of the four C entry points (goat_attn_fwd /
// goat_attn_bwd, goat_attn_long_fwd / goat_attn_long_bwd), the dynamic-LDS opt-in, and the routes from one family into another.
// The device-side tile helpers are in attn_tile.hpp.
#pragma once
#include "common.hpp"

struct AttnArgs {
  const void *Q, *K, *V, *O, *dO;
  void *Ow, *dQ, *dK, *dV;
  int64_t q_rs, q_bs, k_rs, k_bs, v_rs, v_bs, o_rs, o_bs, do_rs, do_bs;
  int64_t dq_rs, dq_bs, dk_rs, dk_bs, dv_rs, dv_bs;
  const float *kmask, *bias;
  float* lse;
  float* dbias;
  int B, nh, Lq, Lk;
  float scale, p;
  uint64_t seed, offset;
  const uint64_t* rng_dev;
};

// attention2.hip; return GOAT_E_SHAPE when the problem is outside their range (the caller then uses the general kernels)
int goat_attn2_fwd(hipStream_t st, const AttnArgs& a);
int goat_attn2_bwd(hipStream_t st, const AttnArgs& a);

// attention.hip: its dQ and dK|dV kernels for a checked problem of any Lk whose K rows fit the LDS (their register arrays do not
// depend on the length; attention_long.hip runs them for Lk <= 512)
int goat_attn_tile_bwd(hipStream_t st, const AttnArgs& a, int dtype);

// the stride rule: rows and samples a whole number of 16-byte chunks apart, the base on a 16-byte boundary
inline bool strides_ok(int dtype, int64_t rs, int64_t bs, const void* ptr) {
  const int epc = dtype == GOAT_BF16 ? 8 : 4;
  return (rs % epc) == 0 && (bs % epc) == 0 && (reinterpret_cast<uintptr_t>(ptr) & 15) == 0;
}

// Forward entry points: the raw arguments in the order of the C ABI, behind the two things in which the entry points differ —
// the largest Lk they serve, and whether O is held to the stride rule (the long forward stores four elements at a time; the short
// forward's general kernels store single elements and take any O).  Checks in the order null pointer -> GOAT_E_ARG, shape ->
// GOAT_E_SHAPE, dtype -> GOAT_E_ARG, strides -> GOAT_E_SHAPE, then fills `a`.
inline int attn_fwd_args(AttnArgs& a, int max_lk, bool check_o, int dtype, const void* Q, int64_t q_rs, int64_t q_bs, const void* K,
                         int64_t k_rs, int64_t k_bs, const void* V, int64_t v_rs, int64_t v_bs, void* O, int64_t o_rs, int64_t o_bs,
                         const float* kmask, const float* bias, float* lse, int B, int nh, int Lq, int Lk, float scale, float p,
                         uint64_t seed, uint64_t offset, const uint64_t* rng_dev) {
  if (!Q || !K || !V || !O || !lse) return GOAT_E_ARG;
  if (B <= 0 || nh <= 0 || Lq <= 0 || Lk <= 0 || Lk > max_lk) return GOAT_E_SHAPE;
  if (dtype != GOAT_F32 && dtype != GOAT_BF16) return GOAT_E_ARG;
  if (!strides_ok(dtype, q_rs, q_bs, Q) || !strides_ok(dtype, k_rs, k_bs, K) || !strides_ok(dtype, v_rs, v_bs, V) ||
      (check_o && !strides_ok(dtype, o_rs, o_bs, O)))
    return GOAT_E_SHAPE;
  a = {};
  a.Q = Q; a.K = K; a.V = V; a.Ow = O;
  a.q_rs = q_rs; a.q_bs = q_bs; a.k_rs = k_rs; a.k_bs = k_bs; a.v_rs = v_rs; a.v_bs = v_bs; a.o_rs = o_rs; a.o_bs = o_bs;
  a.kmask = kmask; a.bias = bias; a.lse = lse;
  a.B = B; a.nh = nh; a.Lq = Lq; a.Lk = Lk; a.scale = scale; a.p = p; a.seed = seed; a.offset = offset; a.rng_dev = rng_dev;
  return 0;
}

// Backward entry points: the forward's operands (O now an input, always held to the stride rule) and the gradient operands behind
// them.  dO and dQ are held to the stride rule; dK and dV are not (the general kernels store single elements; attention2.hip
// checks them for itself).  Same order of checks.
inline int attn_bwd_args(AttnArgs& a, int max_lk, int dtype, const void* Q, int64_t q_rs, int64_t q_bs, const void* K, int64_t k_rs,
                         int64_t k_bs, const void* V, int64_t v_rs, int64_t v_bs, const void* O, int64_t o_rs, int64_t o_bs,
                         const void* dO, int64_t do_rs, int64_t do_bs, void* dQ, int64_t dq_rs, int64_t dq_bs, void* dK, int64_t dk_rs,
                         int64_t dk_bs, void* dV, int64_t dv_rs, int64_t dv_bs, const float* kmask, const float* bias,
                         const float* lse, float* dbias, int B, int nh, int Lq, int Lk, float scale, float p, uint64_t seed,
                         uint64_t offset, const uint64_t* rng_dev) {
  if (!dO || !dQ || !dK || !dV) return GOAT_E_ARG;
  if (int e = attn_fwd_args(a, max_lk, true, dtype, Q, q_rs, q_bs, K, k_rs, k_bs, V, v_rs, v_bs, const_cast<void*>(O), o_rs, o_bs, kmask,
                            bias, const_cast<float*>(lse), B, nh, Lq, Lk, scale, p, seed, offset, rng_dev))
    return e;
  if (!strides_ok(dtype, do_rs, do_bs, dO) || !strides_ok(dtype, dq_rs, dq_bs, dQ)) return GOAT_E_SHAPE;
  a.O = O; a.Ow = nullptr;
  a.dO = dO; a.dQ = dQ; a.dK = dK; a.dV = dV;
  a.do_rs = do_rs; a.do_bs = do_bs; a.dq_rs = dq_rs; a.dq_bs = dq_bs; a.dk_rs = dk_rs; a.dk_bs = dk_bs;
  a.dv_rs = dv_rs; a.dv_bs = dv_bs;
  a.dbias = dbias;
  return 0;
}

// Dynamic LDS above 64 KiB is an opt-in per kernel (hipFuncAttributeMaxDynamicSharedMemorySize).  The attribute is raised only when
// a request exceeds 64 KiB and what was set before: one high-water mark per kernel instantiation and process (the trainers run one
// process per device).
template <auto KERN>
int set_smem(size_t bytes) {
  static size_t cur = 0;
  if (bytes > 64 * 1024 && bytes > cur) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    cur = bytes;
  }
  return 0;
}
