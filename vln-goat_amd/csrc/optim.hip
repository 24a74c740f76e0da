// Fused optimizer step on the gradient arena: goat_grad_sqnorm + goat_adamw_step (pre-training, HF-style AdamW) and goat_optim_step +
// goat_optim_advance (fine-tuning: torch's AdamW / Adam / RMSprop / SGD, every per-step scalar read from device memory) (include/goat_hip.h).
// HBM-bound row kernels: per element 4 B gradient + 8 B moments (read + write) + 4 B parameter (read + write) + 2-4 B shadows,
// 16-byte accesses, one chunk of <= 65536 elements per workgroup so that 208 M parameters are ~3 300 workgroups.
#include "common.hpp"

namespace {

constexpr int CHUNK = 65536;

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ arena, const int64_t* __restrict__ ranges, int n_ranges,
                                                     float* out_sq) {
  // grid-stride over (range, CHUNK-sized piece) pairs
  float acc = 0.f;
  for (int r = 0; r < n_ranges; ++r) {
    const int64_t b = ranges[2 * r], e = ranges[2 * r + 1];
    for (int64_t base = b + (int64_t)blockIdx.x * 1024; base < e; base += (int64_t)gridDim.x * 1024) {
      const int64_t i = base + threadIdx.x * 4;
      if (i + 4 <= e && ((i & 3) == 0)) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(arena + i);
        acc += g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3];
      } else {
        for (int k = 0; k < 4; ++k)
          if (i + k < e) acc += arena[i + k] * arena[i + k];
      }
    }
  }
  acc = wave_sum(acc);
  __shared__ float part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out_sq, part[0] + part[1] + part[2] + part[3]);
}

// One chunk of one tensor, for every update below: the guard, the vector / scalar split, 16-byte loads, `update(g, m, v, p)` on up to four
// elements, 16-byte stores, the three shadow slots and the row-padded store.  Tensor is goat_adamw_tensor or goat_optim_tensor (the members
// used here have the same names in both); m_ is touched only if HAS_M, v_ only if HAS_V.
template <bool HAS_M, bool HAS_V, typename Tensor, typename Update>
__device__ __forceinline__ void walk_chunk(const Tensor& t, int first, const float* __restrict__ grad, float* __restrict__ m_,
                                           float* __restrict__ v_, Update update) {
  const int64_t n = t.numel;
  if (first < 0 || first >= n) return;
  const int64_t end = (int64_t)first + CHUNK < n ? (int64_t)first + CHUNK : n;
  const float* gp = grad + t.arena_off;
  float* mp = HAS_M ? m_ + t.arena_off : nullptr;
  float* vp = HAS_V ? v_ + t.arena_off : nullptr;
  bf16_t* s0 = reinterpret_cast<bf16_t*>(t.shadow0);
  bf16_t* s1 = reinterpret_cast<bf16_t*>(t.shadow1);
  float* sf = t.shadow_f32;
  const bool padded = t.cols > 0;            // shadow0 = row-padded image (leading dimension ld0): scalar stores, tiny tensors
  auto al = [](const void* q, uintptr_t mask) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & mask) == 0; };
  const bool vec = !padded && al(gp, 15) && al(mp, 15) && al(vp, 15) && al(t.param, 15) && al(sf, 15) && al(s0, 7) && al(s1, 7);
  for (int64_t i = first + threadIdx.x * 4; i < end; i += 256 * 4) {
    float g[4], m[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f}, p[4];
    const int cnt = (int)((end - i) < 4 ? (end - i) : 4);
    const bool full = vec && cnt == 4;       // (first and the stride are multiples of 4: i keeps the alignment of the tensor's start)
    if (full) {
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(gp + i), p4 = *reinterpret_cast<const f32x4*>(t.param + i);
      f32x4 m4 = {0.f, 0.f, 0.f, 0.f}, v4 = {0.f, 0.f, 0.f, 0.f};
      if (HAS_M) m4 = *reinterpret_cast<const f32x4*>(mp + i);
      if (HAS_V) v4 = *reinterpret_cast<const f32x4*>(vp + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) { g[k] = g4[k]; m[k] = m4[k]; v[k] = v4[k]; p[k] = p4[k]; }
    } else {
      for (int k = 0; k < cnt; ++k) {
        g[k] = gp[i + k]; p[k] = t.param[i + k];
        if (HAS_M) m[k] = mp[i + k];
        if (HAS_V) v[k] = vp[i + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) update(g[k], m[k], v[k], p[k]);
    if (full) {
      f32x4 m4, v4, p4;
#pragma unroll
      for (int k = 0; k < 4; ++k) { m4[k] = m[k]; v4[k] = v[k]; p4[k] = p[k]; }
      if (HAS_M) *reinterpret_cast<f32x4*>(mp + i) = m4;
      if (HAS_V) *reinterpret_cast<f32x4*>(vp + i) = v4;
      *reinterpret_cast<f32x4*>(t.param + i) = p4;
      bf16x4 b;
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = (bf16_t)p[k];
      if (s0) *reinterpret_cast<bf16x4*>(s0 + i) = b;
      if (s1) *reinterpret_cast<bf16x4*>(s1 + i) = b;
      if (sf) *reinterpret_cast<f32x4*>(sf + i) = p4;
    } else {
      for (int k = 0; k < cnt; ++k) {
        if (HAS_M) mp[i + k] = m[k];
        if (HAS_V) vp[i + k] = v[k];
        t.param[i + k] = p[k];
        if (s0) s0[padded ? ((i + k) / t.cols) * (int64_t)t.ld0 + (i + k) % t.cols : i + k] = (bf16_t)p[k];
        if (s1) s1[i + k] = (bf16_t)p[k];
        if (sf) sf[i + k] = p[k];
      }
    }
  }
}

// The update arithmetic below is compiled with contraction off and names its fused multiply-adds itself (__builtin_fmaf): every product and
// sum rounds where the source says, whatever code surrounds it.  sqrtf and the divisions are the correctly rounded ones.

__global__ __launch_bounds__(256) void adamw_kernel(const float* __restrict__ grad, float* __restrict__ m_, float* __restrict__ v_,
                                                    const goat_adamw_tensor* __restrict__ tensors, const int32_t* __restrict__ chunks,
                                                    float beta1, float beta2, float eps, float max_norm, const float* __restrict__ sq_norm) {
  const goat_adamw_tensor t = tensors[chunks[2 * blockIdx.x]];
  float clip = 1.f;
  if (max_norm > 0.f && sq_norm != nullptr) {
    const float c = max_norm / (sqrtf(*sq_norm) + 1e-6f);        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
    clip = c < 1.f ? c : 1.f;
  }
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  walk_chunk<true, true>(t, chunks[2 * blockIdx.x + 1], grad, m_, v_, [&](float g, float& m, float& v, float& p) {
#pragma clang fp contract(off)
    const float gc = g * clip;
    m = m * beta1 + omb1 * gc;                                   // exp_avg.mul_(beta1).add_(grad, alpha = 1 - beta1)
    v = v * beta2 + omb2 * (gc * gc);                            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) + eps;
    p = __builtin_fmaf(-t.step_size, m / denom, p);              // p.addcdiv_(exp_avg, denom, value = -step_size)
    if (t.decay > 0.f) p = __builtin_fmaf(-t.decay, p, p);       // p.add_(p, alpha = -lr * weight_decay)   (after the update)
  });
}

// What goat_optim_step needs per launch, formed ONCE per thread from the device-resident hyper-parameter block, step counter and squared
// norm.  The double expressions are the ones torch forms on the host (torch/optim/{adamw,adam,rmsprop,sgd}.py, single-tensor path) and
// are rounded to float where torch hands them to a float32 tensor op.
struct OptimScalars {
  float clip, decay_mul, wd, b1, omb1, b2, omb2, eps, neg_step, bc2_sqrt;
};

template <int ALGO>
__device__ __forceinline__ OptimScalars optim_scalars(const goat_optim_hyper* __restrict__ h, const int64_t* __restrict__ step,
                                                      const float* __restrict__ sq_norm) {
#pragma clang fp contract(off)
  OptimScalars s;
  const double lr = h->lr, b1 = h->beta1, b2 = h->beta2, wd = h->weight_decay, max_norm = h->max_norm;
  s.clip = 1.f;
  if (max_norm > 0.0) {
    const float c = (float)max_norm / (sqrtf(*sq_norm) + 1e-6f);        // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
    s.clip = c < 1.f ? c : 1.f;
  }
  s.decay_mul = (float)__builtin_fma(-lr, wd, 1.0);                     // AdamW: param.mul_(1 - lr * weight_decay)
  s.wd = (float)wd;
  s.b1 = (float)b1;
  s.omb1 = (float)(1.0 - b1);
  s.b2 = (float)b2;
  s.omb2 = (float)(1.0 - b2);
  s.eps = (float)h->eps;
  s.neg_step = (float)(-lr);
  s.bc2_sqrt = 1.f;
  if (ALGO == GOAT_OPT_ADAMW || ALGO == GOAT_OPT_ADAM) {
    const double t = (double)(*step + 1);                               // the counter holds the COMPLETED steps
    const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
    s.neg_step = (float)(-(lr / bc1));                                  // step_size = lr / bias_correction1
    s.bc2_sqrt = (float)sqrt(bc2);                                      // bias_correction2 ** 0.5
  }
  return s;
}

// one element; g_raw is the unclipped gradient.  ALGO is a template argument: each instantiation holds one algorithm's arithmetic.
template <int ALGO>
__device__ __forceinline__ void optim_update(float g_raw, float& m, float& v, float& p, const OptimScalars& s) {
#pragma clang fp contract(off)
  float g = g_raw * s.clip;                                             // clip_grad_norm_ multiplies always (by 1.0 when not clipping)
  if (ALGO == GOAT_OPT_ADAMW) p *= s.decay_mul;
  else if (s.wd != 0.f) g = g + s.wd * p;                               // grad.add(param, alpha = weight_decay)
  if (ALGO == GOAT_OPT_ADAMW || ALGO == GOAT_OPT_ADAM) {
    // Which product of a sum rides in the fma is kept as these kernels were first compiled (profiles/optim_fold_isa_diff.txt), hence the
    // two forms per line: AdamW takes grad - exp_avg from the unrounded clip * grad and fuses beta2 * v, Adam fuses the other product.
    const float d = ALGO == GOAT_OPT_ADAMW ? __builtin_fmaf(s.clip, g_raw, -m) : g - m;
    m = s.omb1 < 0.5f ? __builtin_fmaf(s.omb1, d, m) : __builtin_fmaf(-(1.f - s.omb1), d, g);                  // exp_avg.lerp_(grad, 1 - beta1)
    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    v = ALGO == GOAT_OPT_ADAMW ? __builtin_fmaf(v, s.b2, (s.omb2 * g) * g) : __builtin_fmaf(s.omb2 * g, g, v * s.b2);
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;                  // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p + (s.neg_step * m) / denom;                                   // param.addcdiv_(exp_avg, denom, value = -step_size)
  } else if (ALGO == GOAT_OPT_RMSPROP) {
    v = __builtin_fmaf(s.omb1 * g, g, v * s.b1);                        // square_avg.mul_(alpha).addcmul_(grad, grad, value = 1 - alpha)
    p = p + (s.neg_step * g) / (sqrtf(v) + s.eps);                      // param.addcdiv_(grad, square_avg.sqrt().add_(eps), value = -lr)
  } else {
    p = __builtin_fmaf(s.neg_step, g, p);                               // param.add_(grad, alpha = -lr)
  }
}

// m_ is read and written by AdamW / Adam only, v_ by all but SGD (it is RMSprop's square_avg).
template <int ALGO>
__global__ __launch_bounds__(256) void optim_kernel(const float* __restrict__ grad, float* __restrict__ m_, float* __restrict__ v_,
                                                    const goat_optim_tensor* __restrict__ tensors, const int32_t* __restrict__ chunks,
                                                    const goat_optim_hyper* __restrict__ hyper, const int64_t* __restrict__ step,
                                                    const float* __restrict__ sq_norm) {
  constexpr bool HAS_M = ALGO == GOAT_OPT_ADAMW || ALGO == GOAT_OPT_ADAM, HAS_V = ALGO != GOAT_OPT_SGD;
  const goat_optim_tensor t = tensors[chunks[2 * blockIdx.x]];
  const OptimScalars s = optim_scalars<ALGO>(hyper, step, sq_norm);
  walk_chunk<HAS_M, HAS_V>(t, chunks[2 * blockIdx.x + 1], grad, m_, v_,
                           [&](float g, float& m, float& v, float& p) { optim_update<ALGO>(g, m, v, p, s); });
}

// the step's own stream-ordered tail: the counter moves on, the squared norm is kept for last_grad_norm() and cleared for the next
// goat_grad_sqnorm (which accumulates).  One thread: no workgroup of the update kernel, which all read both, ever writes them.
__global__ void optim_advance_kernel(int64_t* step, float* sq_norm, float* last_sq) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *step = *step + 1;
    *last_sq = *sq_norm;
    *sq_norm = 0.f;
  }
}

}  // namespace

extern "C" int goat_grad_sqnorm(void* stream, const float* arena, const int64_t* ranges, int n_ranges, float* out_sq) {
  if (!arena || !ranges || !out_sq || n_ranges < 0) return GOAT_E_ARG;
  if (n_ranges == 0) return 0;
  hipLaunchKernelGGL(sqnorm_kernel, dim3(1024), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arena, ranges, n_ranges, out_sq);
  GOAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int goat_adamw_step(void* stream, const float* grad_arena, float* exp_avg, float* exp_avg_sq, const goat_adamw_tensor* tensors,
                               const int32_t* chunks, int nchunks, float beta1, float beta2, float eps, float max_norm,
                               const float* sq_norm) {
  if (!grad_arena || !exp_avg || !exp_avg_sq || !tensors || !chunks || nchunks < 0) return GOAT_E_ARG;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return GOAT_E_ARG;      // as P/optim/adamw.py:44-51
  if (nchunks == 0) return 0;
  hipLaunchKernelGGL(adamw_kernel, dim3(nchunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), grad_arena, exp_avg, exp_avg_sq,
                     tensors, chunks, beta1, beta2, eps, max_norm, sq_norm);
  GOAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int goat_optim_step(void* stream, int algo, const float* grad_arena, float* exp_avg, float* exp_avg_sq,
                               const goat_optim_tensor* tensors, const int32_t* chunks, int nchunks, const goat_optim_hyper* hyper,
                               const int64_t* step, const float* sq_norm) {
  if (algo != GOAT_OPT_ADAMW && algo != GOAT_OPT_ADAM && algo != GOAT_OPT_RMSPROP && algo != GOAT_OPT_SGD) return GOAT_E_ARG;
  if (!grad_arena || !tensors || !chunks || !hyper || !step || !sq_norm || nchunks < 0) return GOAT_E_ARG;
  if ((algo == GOAT_OPT_ADAMW || algo == GOAT_OPT_ADAM) && !exp_avg) return GOAT_E_ARG;
  if (algo != GOAT_OPT_SGD && !exp_avg_sq) return GOAT_E_ARG;
  if (nchunks == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define GOAT_OPTIM_LAUNCH(A) \
  hipLaunchKernelGGL(optim_kernel<A>, dim3(nchunks), dim3(256), 0, st, grad_arena, exp_avg, exp_avg_sq, tensors, chunks, hyper, step, sq_norm)
  switch (algo) {
    case GOAT_OPT_ADAMW: GOAT_OPTIM_LAUNCH(GOAT_OPT_ADAMW); break;
    case GOAT_OPT_ADAM: GOAT_OPTIM_LAUNCH(GOAT_OPT_ADAM); break;
    case GOAT_OPT_RMSPROP: GOAT_OPTIM_LAUNCH(GOAT_OPT_RMSPROP); break;
    default: GOAT_OPTIM_LAUNCH(GOAT_OPT_SGD); break;
  }
#undef GOAT_OPTIM_LAUNCH
  GOAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int goat_optim_advance(void* stream, int64_t* step, float* sq_norm, float* last_sq) {
  if (!step || !sq_norm || !last_sq) return GOAT_E_ARG;
  hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), step, sq_norm, last_sq);
  GOAT_LAUNCH_CHECK();
  return 0;
}
