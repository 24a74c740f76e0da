// The result stores of the bf16 MFMA GEMM family, written once: the lockstep loop (gemm2_tile.hpp), the ping-pong loop and the
// persistent ping-pong loop (gemm5_tile.hpp) all end in store_tile_f32 or store_tile_bf16.  A wave owns a (32*MI) x (32*NI) patch of C whose
// accumulators are v_mfma_f32_32x32x16_bf16 blocks acc[MI][NI]; everything here works on one wave's patch and needs no workgroup
// barrier.  What a loop chooses is visible at its call site and nowhere else:
//   * where the wave's LDS staging slice is (`wsp`: Staging<NI>::WSLICE bytes no other wave and no LDS-DMA touches);
//   * how far ahead the saved pre-activation is fetched for the x act' epilogues (AHEAD, and PRIMED: block rows the caller requested
//     itself before calling);
//   * whether float32 results are stored non-temporally (NT), and whether the float32 store pins its address arithmetic behind the main loop (PIN).
// Free function templates on purpose: this is the most register-bound code of the tree (the 256 x 256 tiles hold 480 of 512
// registers).  A [&] lambda over the accumulators, defined in every instantiation of the tile, once cost the 256 x 256
// transposed-operand kernels 5 to 162 spilled registers although they never called it, and the grouped weight-gradient launch of
// that tile went from 297 to 446 us (profiles/round3_gemm_spill_check.txt).  (c_row, the MFMA C-layout helper, stays in common.hpp:
// the attention kernels use it too; the argument block G2Args is gemm_args.hpp.)
#pragma once
#include "gemm_args.hpp"

namespace goat_g2 {

// 16-byte result store (inline asm ends in `s_nop 1`: the compiler does not know the statement is a >64-bit VMEM store and would
// otherwise overwrite the data registers inside the store-data hazard window — seen as isolated wrong elements).
// GOAT_G2_STORE: 0 plain, 1 nt (non-temporal), 2 sc1 (write-through: the line leaves the XCD's L2 right
// away instead of in the write-back burst at the end of the kernel, MI355X_MICROARCH.md "publish-large")
#ifndef GOAT_G2_STORE
#define GOAT_G2_STORE 1       // measured: 3840x3072x768 25.9 (plain) -> 21.5 us (nt), 8640x3072x768 64.1 -> 47.7 us
#endif
typedef uint32_t g2_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16(void* dst, const uint4& v) {
#if GOAT_G2_STORE == 1
  const g2_u32x4 q = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(dst), "v"(q) : "memory");
#elif GOAT_G2_STORE == 2
  const g2_u32x4 q = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(q) : "memory");
#else
  *reinterpret_cast<uint4*>(dst) = v;
#endif
}

// One 32-row block row of a wave's patch of the saved pre-activation (bf16, G2Args::aux): CHUNKS 16-byte pieces per lane, rows
// and columns past the problem read as zero.
template <int CHUNKS, int CPR>
__device__ __forceinline__ void load_aux_rows(const G2Args& p, int row_w, int col_w, int lane, uint4* dst) {
  constexpr int EPC = 8;
  const bf16_t* auxp = reinterpret_cast<const bf16_t*>(p.aux);
  const bool vec = auxp != nullptr && (p.ldaux % EPC) == 0 && ((reinterpret_cast<uintptr_t>(auxp) & 15) == 0);
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int idx = c * 64 + lane, r = idx / CPR, cc = idx % CPR;
    const int row = row_w + r, col = col_w + cc * EPC;
    uint4 raw = {0u, 0u, 0u, 0u};
    if (row < p.M) {
      if (col + EPC <= p.N && vec) {
        raw = *reinterpret_cast<const uint4*>(auxp + (int64_t)row * p.ldaux + col);
      } else {
        bf16_t* rv = reinterpret_cast<bf16_t*>(&raw);
        for (int e = 0; e < EPC; ++e)
          if (col + e < p.N) rv[e] = auxp[(int64_t)row * p.ldaux + col + e];
      }
    }
    dst[c] = raw;
  }
}

// A wave's accumulators.  The result stores take them BY VALUE: a tile function that hands `acc` to another function by reference lets the array
// escape until that function is inlined, which is after the first round of per-function optimisation — the main loop of the caller is then
// optimised with the accumulators in memory and comes out different (lockstep 128 x 256 float32 weight gradient: branches around the
// bias-gradient sums inside the K loop, 61.9 against 60.1 us).  By value the caller's copy never escapes; the copy itself disappears with inlining.
template <int MI, int NI> struct AccTile { f32x16 t[MI][NI]; };

// Split-K (ATOMIC: float32 atomic adds, no bias) and float32 results (+ bias; G2Args::accum: C += ...): the plain MFMA operand roles,
// lane = column, registers = rows, so 32 lanes cover 128 contiguous bytes of a row and the accumulators are stored as they are.
// (row0, col0) = first row / column of the wave patch (the same for all lanes of the wave).  NT: results that are not read back here leave through non-temporal stores
// (streamed out of L2, see store16).
template <int MI, int NI, bool ATOMIC, bool NT, bool PIN>
__device__ __forceinline__ void store_tile_f32(const G2Args& p, const AccTile<MI, NI> accs, int row0, int col0, int lane) {
  const f32x16 (&acc)[MI][NI] = accs.t;
  // PIN is a codegen pin, not arithmetic: the empty asm makes the lane index and the patch origin opaque at this point, so that nothing derived
  // from them is computed ahead of the main loop and held in registers across it.  The ping-pong loops set it: without it every float32
  // ping-pong kernel needs one VGPR more than with the store written in place, and pp_group_sk_kernel<256 x 256> — 256 VGPRs, already
  // spilling — goes from 76 to 124 bytes of scratch per lane (lane alone pinned: still 124).  The lockstep loop does not: its code before
  // this header computed the store addresses in FRONT of the main loop, and without the pin it compiles to those instructions again
  // (profiles/gemm_epilogue_fold_resource_usage.txt, gemm_epilogue_fold_ab.txt).  With PIN, row0 / col0 MUST be wave-uniform ("s" constraint).
  if constexpr (PIN) asm volatile("" : "+v"(lane), "+s"(row0), "+s"(col0));
  float* C = reinterpret_cast<float*>(p.C);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = col0 + j * 32 + (lane & 31);
      const float bcol = (!ATOMIC && p.bias != nullptr && col < p.N) ? p.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + i * 32 + c_row(r, lane);
        if (row < p.M && col < p.N) {
          float* dst = C + (int64_t)row * p.ldc + col;
          const float u = acc[i][j][r] + bcol;
          if (ATOMIC) atomicAdd(dst, acc[i][j][r]);
          else if (p.accum) *dst = u + *dst;
          else if (NT) __builtin_nontemporal_store(u, dst);
          else *dst = u;
        }
      }
    }
}

// Geometry of a wave's staging slice for bf16 results: one 32-row block row of the patch, rows padded by 16 bytes (the 8-byte writes
// of 16 rows then hit 16 different bank pairs).  4.5 KiB for 64-column patches, 6.5 KiB for 96.
template <int NI>
struct Staging {
  static constexpr int EPC = 8;                   // bf16 elements per 16-byte chunk
  static constexpr int WCOLS = 32 * NI;
  static constexpr int RBY = WCOLS * 2 + 16;      // row stride in bytes
  static constexpr int WSLICE = 32 * RBY;         // bytes per wave
  static constexpr int CPR = WCOLS / EPC;         // 16-byte chunks per patch row
  static constexpr int CHUNKS = 32 * CPR / 64;    // chunks per lane and block row
  static_assert(32 * CPR % 64 == 0, "a block row is a whole number of 16-byte chunks per lane");
};

constexpr bool epi_is_dact(int epi) { return epi == GOAT_EPI_MUL_DGELU || epi == GOAT_EPI_MUL_DRELU; }
constexpr bool epi_is_act(int epi) { return epi == GOAT_EPI_GELU || epi == GOAT_EPI_RELU; }

// Block rows of the saved pre-activation in flight ahead of their use (x act' epilogues; never touched, hence no registers, in
// every other instantiation).  A caller that requests the first rows itself (PRIMED) owns one of these and fills v[0 .. PRIMED).
template <int NI, int EPI, int AHEAD>
struct AuxAhead {
  static constexpr bool ON = epi_is_dact(EPI) && AHEAD > 0;
  uint4 v[ON ? AHEAD : 1][Staging<NI>::CHUNKS];
};

// bf16 results, every epilogue:  C = act(acc + bias), the bf16 pre-activation optionally saved to `aux` (GELU, RELU);
// C = acc * act'(aux) (MUL_DGELU, MUL_DRELU: no bias — goat_gemm_bf16 rejects one).
// The MFMA operand roles are swapped for these kernels (D = B·A^T, i.e. lane = row of C, the 16 registers of a block = 4 groups of
// 4 consecutive columns), so a lane packs 4 results into 8 bytes.  Each wave stages one 32-row block row of its patch at a time
// through its OWN slice `wsp` of LDS — no workgroup barrier: a wave starts storing the moment its last MFMA retires — and
// writes it out as whole rows of the patch (128-B / 192-B segments, 16 B per lane; columns past N and rows past M are dropped,
// a C or aux that is not 16-byte addressable is written element by element).  Round 1 staged the whole tile with 2-byte LDS
// writes between two __syncthreads(): 9.6 of the 26.8 us of the 3840x3072x768 launch (profiles/round2_gemm_epilogue_ab.txt).
//
// x act' epilogues (FFN dgrad): the saved pre-activation of block row i travels registers -> slice -> each lane's own 4-column
// groups.  AHEAD (clamped to MI) block rows of it are in flight at any time: rows [PRIMED, AHEAD) are requested on entry, row
// i + AHEAD as soon as row i has been handed to the slice, so one HBM round trip per tile is exposed instead of one per block
// row (fetching each row where it is used: 399 TFLOP/s on 3840 x 3072 x 768 against 548 without the multiply; 20480 x 3072 x 768
// ping-pong 548 against 771 with the GELU epilogue).  Every row in flight costs 4 * CHUNKS registers per lane.  AHEAD = 0: nothing is
// held, every 16-byte piece is fetched right where it is written to the slice (tiles whose accumulators leave no room).
template <int MI, int NI, int EPI, int AHEAD, int PRIMED>
__device__ __forceinline__ void store_tile_bf16(const G2Args& p, const AccTile<MI, NI> accs, char* wsp, int row0, int col0, int lane,
                                                AuxAhead<NI, EPI, AHEAD>& ahead) {
  const f32x16 (&acc)[MI][NI] = accs.t;
  typedef bf16_t T;
  typedef Staging<NI> S;
  constexpr int EPC = S::EPC, RBY = S::RBY, CPR = S::CPR, CHUNKS = S::CHUNKS;
  constexpr bool DACT = epi_is_dact(EPI), ACT = epi_is_act(EPI);
  constexpr int AD = AHEAD < MI ? AHEAD : MI;
  static_assert(AHEAD >= 0 && AHEAD <= 3 && PRIMED >= 0 && PRIMED <= AD, "prefetch policy: 0..3 block rows ahead, the first PRIMED of them by the caller");
  const int hi = lane >> 5, l31 = lane & 31;
  T* aux = reinterpret_cast<T*>(p.aux);
  T* C = reinterpret_cast<T*>(p.C);
  const bool c_vec = (p.ldc % EPC) == 0 && ((reinterpret_cast<uintptr_t>(C) & 15) == 0);
  const bool aux_vec = aux != nullptr && (p.ldaux % EPC) == 0 && ((reinterpret_cast<uintptr_t>(aux) & 15) == 0);
  // bias of this lane's columns: block j, group q -> columns j*32 + 4*hi + 8*q + {0..3}
  f32x4 bv[DACT ? 1 : NI][4];
  if (!DACT) {
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = col0 + j * 32 + 4 * hi + 8 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[j][q][e] = (p.bias != nullptr && col + e < p.N) ? p.bias[col + e] : 0.f;
      }
  }
  if constexpr (DACT) {
#pragma unroll
    for (int i = PRIMED; i < AD; ++i) load_aux_rows<CHUNKS, CPR>(p, row0 + i * 32, col0, lane, ahead.v[i]);
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row_w = row0 + i * 32;                       // first row of this block row
    if constexpr (DACT) {
#pragma unroll
      for (int c = 0; c < CHUNKS; ++c) {
        const int idx = c * 64 + lane, r = idx / CPR, cc = idx % CPR;
        uint4 now;
        if constexpr (AD > 0) now = ahead.v[i % AD][c];
        else load_aux_rows<1, CPR>(p, row_w, col0, idx, &now);     // (chunk c of this lane = chunk 0 of "lane" idx)
        *reinterpret_cast<uint4*>(wsp + r * RBY + cc * 16) = now;
      }
      if constexpr (AD > 0) {
        if (i + AD < MI) load_aux_rows<CHUNKS, CPR>(p, row_w + AD * 32, col0, lane, ahead.v[i % AD]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same-wave LDS hand-over between lanes
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        char* slot = wsp + l31 * RBY + (j * 32 + 4 * hi + 8 * q) * 2;
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = DACT ? acc[i][j][4 * q + e] : acc[i][j][4 * q + e] + bv[DACT ? 0 : j][q][e];
        if (DACT) {
          const bf16x4 a4 = *reinterpret_cast<const bf16x4*>(slot);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float av = (float)a4[e];
            u[e] = (EPI == GOAT_EPI_MUL_DGELU) ? u[e] * dgelu_fast(av) : (av > 0.f ? u[e] : 0.f);
          }
        }
        bf16x4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (bf16_t)u[e];
        *reinterpret_cast<bf16x4*>(slot) = o4;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // same-wave LDS hand-over between lanes
    // write-out: whole patch rows, 16 bytes per lane.  Activation epilogues store the staged pre-activation to `aux` (if
    // given) and the activation of the same bf16 values to C from this one pass.
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int idx = c * 64 + lane, r = idx / CPR, cc = idx % CPR;
      const int row = row_w + r, col = col0 + cc * EPC;
      uint4 raw = *reinterpret_cast<const uint4*>(wsp + r * RBY + cc * 16);
      if (row >= p.M || col >= p.N) continue;
      if (ACT) {
        if (aux != nullptr) {
          if (col + EPC <= p.N && aux_vec) {
            store16(aux + (int64_t)row * p.ldaux + col, raw);
          } else {
            const T* rv = reinterpret_cast<const T*>(&raw);
            for (int e = 0; e < EPC; ++e)
              if (col + e < p.N) aux[(int64_t)row * p.ldaux + col + e] = rv[e];
          }
        }
        bf16x8 v = *reinterpret_cast<bf16x8*>(&raw);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const float u = (float)v[e];
          const float h = (EPI == GOAT_EPI_GELU) ? gelu_fast(u) : fmaxf(u, 0.f);
          v[e] = (bf16_t)h;
        }
        raw = *reinterpret_cast<uint4*>(&v);
      }
      if (col + EPC <= p.N && c_vec) {
        store16(C + (int64_t)row * p.ldc + col, raw);
      } else {
        const T* rv = reinterpret_cast<const T*>(&raw);
        for (int e = 0; e < EPC; ++e)
          if (col + e < p.N) C[(int64_t)row * p.ldc + col + e] = rv[e];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the slice is rewritten by the next block row
  }
}
// ... with nothing requested by the caller
template <int MI, int NI, int EPI, int AHEAD>
__device__ __forceinline__ void store_tile_bf16(const G2Args& p, const AccTile<MI, NI> accs, char* wsp, int row0, int col0, int lane) {
  AuxAhead<NI, EPI, AHEAD> ahead;
  store_tile_bf16<MI, NI, EPI, AHEAD, 0>(p, accs, wsp, row0, col0, lane, ahead);
}

}  // namespace goat_g2
