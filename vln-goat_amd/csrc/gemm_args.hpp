// Argument block of one bf16 MFMA GEMM problem (goat_gemm_bf16 / goat_wgrad_grouped): what the main loops (gemm2_tile.hpp, gemm5_tile.hpp) and
// the result stores (gemm_epilogue.hpp) read on the device.
#pragma once
#include "common.hpp"

namespace goat_g2 {

struct G2Args {
  const void* A; const void* B; void* C; const float* bias; void* aux;
  int64_t lda, ldb, ldc, ldaux;
  int M, N, Kc;
  int tiles_m, tiles_n;
  int k_tiles_per_split;
  uint32_t a_bytes, b_bytes;  // buffer sizes for the bounds check
  float* colsum;              // TA only: colsum[m] += sum_k A[k,m]  (bias gradient fused into wgrad)
  int accum;                  // f32 output, no split: C += A·B (read-modify-write) instead of C = A·B
  int group_m;                // tile order: column-major inside groups of group_m tile rows (L2-sized 2-D blocks per XCD)
};

}  // namespace goat_g2
