// Element-wise dropout kernels: dropout (+ residual add) forward / backward and the backward of dropout(act(u)).
#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------ dropout (+add)
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                      int64_t n, float p, uint64_t seed, uint64_t offset,
                                                      const uint64_t* __restrict__ rng_dev) {
  constexpr int EPC = DT<T>::EPC;
  const DropMask drop(p, seed, offset, rng_dev);
  const int64_t nchunk = n / EPC;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nchunk; c += (int64_t)gridDim.x * blockDim.x) {
    Chunk<T> v;
    v.load(x + c * EPC);
    if (drop.on) {
      const uint32_t km = drop.bits<EPC>(c * EPC);
#pragma unroll
      for (int e = 0; e < EPC; ++e) v.v[e] = ((km >> e) & 1u) ? v.v[e] * drop.ks : 0.f;
    }
    if (!BWD && res) v.add(res + c * EPC);
    v.store_stream(y + c * EPC);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (n - nchunk * EPC)) {
    const int64_t i = nchunk * EPC + threadIdx.x;
    float v = to_f(x[i]);
    drop.apply(v, i);
    if (!BWD && res) v += to_f(res[i]);
    y[i] = from_f<T>(v);
  }
}


// ------------------------------------------------------------------------------------ activation backward
// dx = dropmask(dy) * act'(u)   (act: 1 gelu, 2 relu): backward of  h = dropout_p(act(u)).
template <typename T>
__global__ __launch_bounds__(256) void act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ u, T* __restrict__ dx,
                                                      int64_t n, int act, float p, uint64_t seed, uint64_t offset,
                                                      const uint64_t* __restrict__ rng_dev) {
  constexpr int EPC = DT<T>::EPC;
  const DropMask drop(p, seed, offset, rng_dev);
  const int64_t nchunk = n / EPC;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nchunk; c += (int64_t)gridDim.x * blockDim.x) {
    Chunk<T> d, uu;
    d.load(dy + c * EPC);
    uu.load(u + c * EPC);
    const uint32_t km = drop.on ? drop.bits<EPC>(c * EPC) : 0xFFFFFFFFu;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      float g = d.v[e];
      if (drop.on) g = ((km >> e) & 1u) ? g * drop.ks : 0.f;
      g *= (act == 1) ? dgelu_f(uu.v[e]) : (uu.v[e] > 0.f ? 1.f : 0.f);
      d.v[e] = g;
    }
    d.store_stream(dx + c * EPC);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - nchunk * EPC)) {
    const int64_t i = nchunk * EPC + threadIdx.x;
    float g = to_f(dy[i]);
    const float uv = to_f(u[i]);
    drop.apply(g, i);
    g *= (act == 1) ? dgelu_f(uv) : (uv > 0.f ? 1.f : 0.f);
    dx[i] = from_f<T>(g);
  }
}

// grid of the three launches: 256-thread blocks, one per 256 items of 8 elements, 1 .. 2048 of them
int chunk_walk_blocks(int64_t n) {
  const int64_t blocks = (n / 8 + 255) / 256;
  return (int)(blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks);
}

}  // namespace

extern "C" int goat_dropout_add_fwd(void* stream, int dtype, const void* x, const void* residual, void* y, int64_t n,
                                    float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev) {
  if (!x || !y) return GOAT_E_ARG;
  if (n <= 0) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL((dropout_kernel<T, false>), dim3(chunk_walk_blocks(n)), dim3(256), 0, ST(stream), (const T*)x, (const T*)residual, (T*)y, n, p,
                       seed, offset, rng_dev);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_dropout_bwd(void* stream, int dtype, const void* dy, void* dx, int64_t n, float p, uint64_t seed,
                                uint64_t offset, const uint64_t* rng_dev) {
  if (!dy || !dx) return GOAT_E_ARG;
  if (n <= 0) return GOAT_E_SHAPE;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL((dropout_kernel<T, true>), dim3(chunk_walk_blocks(n)), dim3(256), 0, ST(stream), (const T*)dy, (const T*)nullptr, (T*)dx, n, p,
                       seed, offset, rng_dev);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int goat_act_bwd(void* stream, int dtype, const void* dy, const void* u, void* dx, int64_t n, int act,
                            float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev) {
  if (!dy || !u || !dx) return GOAT_E_ARG;
  if (n <= 0) return GOAT_E_SHAPE;
  if (act != GOAT_EPI_GELU && act != GOAT_EPI_RELU) return GOAT_E_ARG;
  return dtype_dispatch(dtype, [&](auto dt) -> int {
    typedef GOAT_DT_TYPE(dt) T;
    hipLaunchKernelGGL(act_bwd_kernel<T>, dim3(chunk_walk_blocks(n)), dim3(256), 0, ST(stream), (const T*)dy, (const T*)u, (T*)dx, n, act, p, seed,
                       offset, rng_dev);
    GOAT_LAUNCH_CHECK();
    return 0;
  });
}
