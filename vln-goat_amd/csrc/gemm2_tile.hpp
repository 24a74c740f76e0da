// Device code of goat_gemm_bf16 / goat_wgrad_grouped: one pipelined bf16 MFMA GEMM tile for gfx950 with direct-to-LDS loads,
// all three operand layouts, for a family of workgroup tiles.  Included by gemm2.hip (4-wave tiles, 128-column tiles, the C
// entry points) and gemm3.hip (the 8-wave 192/256-wide tiles), which are compiled in parallel.
//
//   C[M,N] = epilogue( op(A) · op(B)^T )        contraction length Kc
//     TA=0: A is [M, Kc] (Kc contiguous)        TA=1: A is [Kc, M] (M contiguous)   -> "transposed" operand
//     TB=0: B is [N, Kc]                        TB=1: B is [Kc, N]
//   (TA,TB) = (0,0) forward  y = x W^T ; (0,1) dgrad  dx = dy W ; (1,1) wgrad  dW = dy^T x.
//
// Every operand K-tile goes L2 -> LDS by `buffer_load ... lds` (LDS-DMA, no VGPR round trip) into a ring of NSTAGE stages
// with NSTAGE-1 tiles in flight across a single raw s_barrier per K-tile and counted vmcnt waits; out-of-range rows /
// contraction tails are zero-filled by the buffer descriptor's bounds check.  LDS images are lane-linear (DMA constraint), so
// bank conflicts are removed by XOR-swizzling the *source* address and applying the same involution on the fragment reads.
// Transposed operands are read with ds_read_b64_tr_b16 (hardware 4x16 transpose), so wgrad/dgrad need no transposed copies.
// LDS reads are inline asm (hipcc would otherwise drain the DMA queue with vmcnt(0) before every ds_read).
//
// Tile family (Cfg<WM, WN, MI, NI>): WM x WN waves, each wave a (32*MI) x (32*NI) patch of v_mfma_f32_32x32x16_bf16 blocks,
// BM = 32*MI*WM rows, BN = 32*NI*WN columns, BK = 64.  Why the big tiles: scripts/l2_lds_bw.hip measures what a CU can pull
// from its XCD's L2 into LDS at 50-58 B/clk when the data is L2-resident and 18-40 B/clk when it comes from the Infinity
// Cache; at the MFMA peak a 128x128 tile consumes 64 B/clk, 256x128 48, 192x256 37, 256x256 32 (profiles/round2_l2_lds_bw.txt).
//
// The result stores are gemm_epilogue.hpp's (shared with the ping-pong loops).  This loop's choices: every wave stages through slice
// `wave` of the drained ring; block row 0 of the saved pre-activation of the x act' epilogues is requested before the drain barrier and two
// block rows are kept in flight where the accumulators leave room (none otherwise); float32 stores follow GOAT_G2_STORE.
// (A deliberate change of schedule, the only one of the move into the shared header: this loop used to hold the same two buffers but request
// block row i + 1 at the top of block row i; now row i + 2 goes out as soon as row i has been handed to LDS, and the wait for row i + 1 no
// longer covers the result stores of row i.  Same registers, same results; 3840 x 3072 x 768 x GELU' 27.2 -> 26.9 us on 192 x 256, 29.9 -> 29.1 on
// 128 x 128 x 8 waves, profiles/gemm_epilogue_fold_ab.txt.)
#pragma once
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>
#include "gemm_epilogue.hpp"
#include "gemm_tiles.hpp"

namespace goat_g2 {

constexpr int BK = 64;
#ifndef GOAT_GEMM_FRAG_DEPTH
#define GOAT_GEMM_FRAG_DEPTH 2
#endif
#ifndef GOAT_G2_ROTATED       // 1: barrier at the top of a K-tile's last k-step (see the main loop); 0: barrier between K-tiles.
#define GOAT_G2_ROTATED 0     // Measured (profiles/round2_gemm_epilogue_ab.txt): equal on the 192/256-wide tiles at K = 768, 3-12 % slower on
#endif                        // the 128-wide and 3-4-stage configurations, 5 % faster only at 8192^3: the plain order is the default
#ifndef GOAT_G2_SPREAD        // rotated loop: k-steps over which a tile's LDS-DMA instructions are issued (1..3)
#define GOAT_G2_SPREAD 1
#endif
#ifndef GOAT_G2_SETPRIO       // s_setprio 1 around every MFMA cluster
#define GOAT_G2_SETPRIO 0
#endif
#ifndef GOAT_G2_NOEPI         // experiments only: skip the epilogue (stores nothing)
#define GOAT_G2_NOEPI 0
#endif
#ifndef GOAT_G2_TIMING        // experiments only: per-wave cycle sums {wait for DMA + last fragments, barrier, compute phase, total}
#define GOAT_G2_TIMING 0      // written to `aux` as uint32[(block * waves + wave) * 4 ..] (call with epilogue NONE and an aux buffer)
#endif

template <int WM_, int WN_, int MI_, int NI_>
struct Cfg {
  static constexpr int WM = WM_, WN = WN_, MI = MI_, NI = NI_;
  static constexpr int NW = WM * WN, NTH = NW * 64;
  static constexpr int BM = 32 * MI * WM, BN = 32 * NI * WN;
  static constexpr bool EIGHT = BM == 128 && BN == 128 && NW == 8;      // the tile GOAT_GEMM_8WAVES selects
};
// tile ids of the C ABI (bm | bn << 16; bn = 0 means 128; GOAT_GEMM_8WAVES in nstage selects the 8-wave 128x128 tile)
typedef Cfg<2, 2, 1, 2> T64;        //  64 x 128, 4 waves
typedef Cfg<2, 2, 2, 2> T128;       // 128 x 128, 4 waves
typedef Cfg<4, 2, 1, 2> T128X8;     // 128 x 128, 8 waves (32x64 wave patches: twice the waves issue the tile's LDS-DMA)
typedef Cfg<4, 2, 2, 2> T256;       // 256 x 128, 8 waves
typedef Cfg<2, 4, 2, 2> T128x256;   // 128 x 256, 8 waves
typedef Cfg<2, 4, 3, 2> T192x256;   // 192 x 256, 8 waves  (M = 3840 = 20 x 192: 240 tiles at N = 3072)
typedef Cfg<4, 2, 2, 3> T256x192;   // 256 x 192, 8 waves  (N = 2304 = 12 x 192)
typedef Cfg<2, 4, 4, 2> T256x256;   // 256 x 256, 8 waves
typedef Cfg<2, 3, 3, 2> T192x192;   // 192 x 192, SIX waves (3840 x 2304: 20 x 12 = 240 tiles — one round on 256 CUs; 256 x 192 gives 180)
typedef Cfg<1, 4, 3, 1> T96;        //  96 x 128, 4 waves  (M = 3840 = 40 x 96: 240 tiles at N = 768 — one round on 256 CUs, against 180 tiles of 128 x 128)

typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ uint4 lds_read_b128(uint32_t addr) {
  uint4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}
__device__ __forceinline__ uint2 lds_read_tr16(uint32_t addr) {
  uint2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}
template <int N_> __device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N_) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N_> __device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}
// Per-operand tile geometry.  ROWS x RB bytes, lane-linear LDS image, swizzled source.
template <bool T, int BMN>
struct Tile {
  static constexpr int RB = T ? BMN * 2 : BK * 2;         // bytes per LDS row
  static constexpr int ROWS = T ? BK : BMN;
  static constexpr int BYTES = ROWS * RB;                 // 16 KiB (BMN=128) / 8 KiB (BMN=64) / 32 KiB (BMN=256)
  static constexpr int NINST = BYTES / 1024;              // DMA wave-instructions per tile
  static constexpr int RPB = 256 / RB > 0 ? 256 / RB : 1; // LDS rows per 256-B bank row
  static constexpr int C64 = RB / 64;                     // 64-B chunks per row
  static_assert(!T || (C64 & (C64 - 1)) == 0, "transposed operand tiles need a power-of-two width (XOR swizzle of 64-B chunks)");

  // byte offset inside the *matrix* (global) for LDS linear offset o of the tile whose origin is (mn0, k0=0)
  __device__ static __forceinline__ uint32_t src_off(int o, int mn0, int64_t ld) {
    const int row = o / RB, slot = (o % RB) >> 4;
    if (!T) {
      const int c = slot ^ ((row >> 1) & 7);
      return (uint32_t)(((int64_t)(mn0 + row) * ld + c * 8) * 2);
    } else {
      const int c64 = (slot >> 2) ^ ((row / RPB) % C64);
      const int col = ((c64 << 2) | (slot & 3)) * 8;
      return (uint32_t)(((int64_t)row * ld + mn0 + col) * 2);
    }
  }
  // per-K-tile advance of the source offset in bytes
  __device__ static __forceinline__ uint32_t k_step(int64_t ld) { return T ? (uint32_t)(BK * ld * 2) : (uint32_t)(BK * 2); }
};

// fragment read addresses --------------------------------------------------------------------------
// non-transposed: lane (l31,hi) reads 16-B chunk (ks*2+hi) of row `row` -> slot = chunk ^ ((row>>1)&7)
__device__ __forceinline__ uint32_t frag_addr_n(uint32_t tile_base, int row, int ks, int hi) {
  return tile_base + row * (BK * 2) + ((((ks << 1) | hi) ^ ((row >> 1) & 7)) << 4);
}
// transposed: two ds_read_b64_tr_b16; `col0` = first column of this lane's 16-column block,
// t = lane&15 supplies the address of k-row (kbase + (t>>2)), columns col0 + 4*(t&3) .. +3
template <int RB, int RPB, int C64>
__device__ __forceinline__ uint32_t frag_addr_t(uint32_t tile_base, int kr, int col) {
  const int byte = col * 2;
  const int slot = byte >> 4;
  const int c64 = (slot >> 2) ^ ((kr / RPB) % C64);
  return tile_base + kr * RB + ((((c64 << 2) | (slot & 3))) << 4) + (byte & 15);
}

// blockIdx.x -> position in an order that gives every XCD (8 private L2s, workgroups dealt round-robin) ONE contiguous chunk
__device__ __forceinline__ int xcd_chunk_position(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// position in a problem's tile order -> (tile row, tile column).  Tiles are visited column-major within groups of group_m tile rows, so the
// workgroups an XCD runs at a time (xcd_chunk_position) cover a compact group_m x (n / group_m) block: its A and B panels are fetched into that
// L2 once, and the 8 XCD chunks form a 2-D partition of C instead of 8 full-width stripes.
__device__ __forceinline__ void tile_of_position(const G2Args& p, int pos, int& tm, int& tn) {
  const int gsz = p.group_m * p.tiles_n;
  const int grp = pos / gsz, gi = pos - grp * gsz;
  const int gm = min(p.tiles_m - grp * p.group_m, p.group_m);
  tn = gi / gm;
  tm = grp * p.group_m + (gi - tn * gm);
}

template <class CF, bool TA, bool TB, int NSTAGE>
constexpr int smem_bytes() { return NSTAGE * (Tile<TA, CF::BM>::BYTES + Tile<TB, CF::BN>::BYTES); }

// One output tile of one GEMM problem.  `bid` = position of the tile in the problem's tile order, `split` = K-split index.
template <class CF, bool TA, bool TB, typename OutT, int EPI, bool SPLITK, int NSTAGE>
__device__ __forceinline__ void gemm2_tile(const G2Args& p, int bid, int split) {
#if defined(__HIP_DEVICE_COMPILE__)  // (host pass: the gfx950-only builtins below would silently drop the kernel stubs)
  constexpr int BM = CF::BM, BN = CF::BN, MI = CF::MI, NI = CF::NI, NW = CF::NW, NTH = CF::NTH, WN = CF::WN;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef Tile<TA, BM> TLA;
  typedef Tile<TB, BN> TLB;
  constexpr int STAGE = TLA::BYTES + TLB::BYTES;
  constexpr int WROWS = 32 * MI, WCOLS = 32 * NI;       // the wave patch
  constexpr int IPWA = TLA::NINST / NW, IPWB = TLB::NINST / NW;   // DMA wave-instructions per wave and K-tile
  static_assert(IPWA >= 1 && IPWB >= 1 && IPWA * NW == TLA::NINST && IPWB * NW == TLB::NINST,
                "every wave issues a whole number (>= 1) of DMA instructions per operand");
  constexpr int LOADS = IPWA + IPWB;
  constexpr int KSTEPS = BK / 16;
  // Where a K-tile's DMA instructions are issued: deep rings (>= 3 stages) have a whole K-tile of slack, so the instructions
  // go behind the MFMAs of all four k-steps (each costs the issuing wave ~60-100 cycles); a 2-stage ring waits for the tile
  // at the very next barrier.  There the small tiles issue everything right after the barrier (measured +4...+17 % if
  // spread), the big ones (>= 2048 MFMA cycles per K-tile) spread over the first two k-steps.
  constexpr bool BIG = (MI * NI >= 6);
  constexpr bool INTERLEAVE = NSTAGE >= 3 || BIG;
  constexpr int SPREAD = NSTAGE >= 3 ? KSTEPS : 2;
  // fragment prefetch distance in k-steps (each k-step's fragments have their own registers); bounded by the 4-bit lgkmcnt
  constexpr bool SWAP = !SPLITK && sizeof(OutT) == 2;                  // bf16 results: swapped MFMA operand roles (see the epilogue)
  constexpr int RD = MI * (TA ? 2 : 1) + NI * (TB ? 2 : 1);            // ds_read instructions per k-step
  // (the counted wait in front of k-step ks allows (FD-1)*RD reads to stay in flight: THAT must fit the 4-bit lgkmcnt; with more
  // than 15 reads issued the wave simply stalls at issue.  Round 1 required FD*RD <= 15 and ran every transposed-operand tile
  // — all weight gradients — one k-step ahead only.)
  // RD = 16 (the 4 x 4 patch with both operands transposed): one k-step ahead, the wait count clamped to 15 — LDS reads return
  // in order, so waiting for "at most 15 outstanding" completes every read of the current k-step and the first of the next.
  constexpr int FD = RD == 16 ? 2 : ((GOAT_GEMM_FRAG_DEPTH - 1) * RD <= 15) ? GOAT_GEMM_FRAG_DEPTH : (15 / RD + 1 >= 1 ? (15 / RD + 1 < 3 ? 15 / RD + 1 : 3) : 1);
  static_assert(RD <= 16 && ((FD - 1) * RD <= 15 || RD == 16), "the reads a counted wait leaves in flight must fit the lgkmcnt counter");

  // `wave` through readfirstlane: the compiler then keeps every wave-uniform quantity (the LDS addresses of this wave's DMA
  // pieces, hence M0) in SGPRs instead of a v_add + v_readfirstlane + s_mov chain in front of every buffer_load ... lds
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int hi = lane >> 5, l31 = lane & 31;

  int tm, tn;       // `bid` walks a contiguous chunk per XCD (each XCD has its own L2)
  tile_of_position(p, bid, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  int kt_begin = 0, kt_end = (p.Kc + BK - 1) / BK;
  if (SPLITK) {
    kt_begin = split * p.k_tiles_per_split;
    kt_end = min(kt_end, kt_begin + p.k_tiles_per_split);
    if (kt_begin >= kt_end) return;
  }
  const int nkt = kt_end - kt_begin;

  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, (int)p.a_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.B), 0, (int)p.b_bytes, 0x00020000);

  // per-lane source offsets of this wave's DMA instructions at k-tile 0 of this split
  uint32_t offa[IPWA], offb[IPWB];
  const uint32_t ka = TLA::k_step(p.lda), kb = TLB::k_step(p.ldb);
#pragma unroll
  for (int j = 0; j < IPWA; ++j)
    offa[j] = TLA::src_off((wave * IPWA + j) * 1024 + lane * 16, m0, p.lda) + (uint32_t)kt_begin * ka;
#pragma unroll
  for (int j = 0; j < IPWB; ++j)
    offb[j] = TLB::src_off((wave * IPWB + j) * 1024 + lane * 16, n0, p.ldb) + (uint32_t)kt_begin * kb;

#define GOAT_ISSUE(t_)                                                                                              \
  do {                                                                                                              \
    char* st_ = smem + ((t_) % NSTAGE) * STAGE;                                                                     \
    const uint32_t sa_ = (uint32_t)(t_) * ka, sb_ = (uint32_t)(t_) * kb;                                            \
    _Pragma("unroll") for (int j = 0; j < IPWA; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(                  \
        ra, (lds_void*)(st_ + (wave * IPWA + j) * 1024), 16, offa[j], sa_, 0, 0);                               \
    _Pragma("unroll") for (int j = 0; j < IPWB; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(                  \
        rb, (lds_void*)(st_ + TLA::BYTES + (wave * IPWB + j) * 1024), 16, offb[j], sb_, 0, 0);                  \
  } while (0)
  // one DMA wave-instruction (number j_ of this wave's LOADS) of K-tile t_
#define GOAT_ISSUE_ONE(t_, j_)                                                                                      \
  do {                                                                                                              \
    char* st_ = smem + ((t_) % NSTAGE) * STAGE;                                                                     \
    if ((j_) < IPWA)                                                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(st_ + (wave * IPWA + (j_)) * 1024), 16,          \
                                               offa[(j_) < IPWA ? (j_) : 0], (uint32_t)(t_) * ka, 0, 0);        \
    else                                                                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void*)(st_ + TLA::BYTES + (wave * IPWB + (j_) - IPWA) * 1024), 16, \
                                               offb[(j_) >= IPWA ? (j_) - IPWA : 0], (uint32_t)(t_) * kb, 0, 0); \
  } while (0)

  AccTile<MI, NI> accs;
  f32x16 (&acc)[MI][NI] = accs.t;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const uint32_t smem_base = (uint32_t)(uintptr_t)(lds_void*)smem;  // LDS byte offset of the dynamic region
  const int t15 = lane & 15, g = lane >> 4;
  const bool do_colsum = TA && p.colsum != nullptr && tn == 0 && wn == 0;
  float bsum[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) bsum[i] = 0.f;
  bf16x8 fa[KSTEPS][MI], fb[KSTEPS][NI];

  // fragments of k-step ks_ of the stage at (sa_, sb_) -> fa[buf_], fb[buf_]
#define GOAT_LOAD_FRAGS(sa_, sb_, ks_, buf_)                                                                         \
  do {                                                                                                              \
    _Pragma("unroll") for (int i = 0; i < MI; ++i) {                                                                \
      if (!TA) {                                                                                                    \
        uint4 v = lds_read_b128(frag_addr_n((sa_), wm * WROWS + i * 32 + l31, (ks_), hi));                        \
        fa[buf_][i] = *reinterpret_cast<bf16x8*>(&v);                                                               \
      } else {                                                                                                      \
        const int col = wm * WROWS + i * 32 + (g & 1) * 16 + (t15 & 3) * 4;                                      \
        const int kr = (ks_) * 16 + 8 * (g >> 1) + (t15 >> 2);                                                      \
        uint2 v0 = lds_read_tr16(frag_addr_t<TLA::RB, TLA::RPB, TLA::C64>((sa_), kr, col));                         \
        uint2 v1 = lds_read_tr16(frag_addr_t<TLA::RB, TLA::RPB, TLA::C64>((sa_), kr + 4, col));                     \
        uint4 v = {v0.x, v0.y, v1.x, v1.y};                                                                         \
        fa[buf_][i] = *reinterpret_cast<bf16x8*>(&v);                                                               \
      }                                                                                                             \
    }                                                                                                               \
    _Pragma("unroll") for (int j = 0; j < NI; ++j) {                                                                \
      if (!TB) {                                                                                                    \
        uint4 v = lds_read_b128(frag_addr_n((sb_), wn * WCOLS + j * 32 + l31, (ks_), hi));                          \
        fb[buf_][j] = *reinterpret_cast<bf16x8*>(&v);                                                               \
      } else {                                                                                                      \
        const int col = wn * WCOLS + j * 32 + (g & 1) * 16 + (t15 & 3) * 4;                                         \
        const int kr = (ks_) * 16 + 8 * (g >> 1) + (t15 >> 2);                                                      \
        uint2 v0 = lds_read_tr16(frag_addr_t<TLB::RB, TLB::RPB, TLB::C64>((sb_), kr, col));                         \
        uint2 v1 = lds_read_tr16(frag_addr_t<TLB::RB, TLB::RPB, TLB::C64>((sb_), kr + 4, col));                     \
        uint4 v = {v0.x, v0.y, v1.x, v1.y};                                                                         \
        fb[buf_][j] = *reinterpret_cast<bf16x8*>(&v);                                                               \
      }                                                                                                             \
    }                                                                                                               \
  } while (0)
#define GOAT_MMA(ks_)                                                                                              \
  do {                                                                                                              \
    if (TA && do_colsum) {       /* bias gradient: v_dot2c_f32_bf16 (pair . (1, 1) + acc), four per fragment instead of eight conversions + eight adds (round 6) */ \
      _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                                \
        _Pragma("unroll") for (int e2 = 0; e2 < 4; ++e2) {                                                          \
          const bf16x2 pr_ = {fa[ks_][i][2 * e2], fa[ks_][i][2 * e2 + 1]};                                          \
          bsum[i] = __builtin_amdgcn_fdot2_f32_bf16(pr_, bf16x2{(bf16_t)1.0f, (bf16_t)1.0f}, bsum[i], false);       \
        }                                                                                                           \
    }                                                                                                               \
    if (GOAT_G2_SETPRIO) __builtin_amdgcn_s_setprio(1);                                                             \
    _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                                  \
      _Pragma("unroll") for (int j = 0; j < NI; ++j) {                                                              \
        if (SWAP) mma32(acc[i][j], fb[ks_][j], fa[ks_][i]);   /* lane = row of C, registers = columns (bf16 epilogue) */ \
        else mma32(acc[i][j], fa[ks_][i], fb[ks_][j]);        /* lane = column, registers = rows (f32 stores / atomics) */ \
      }                                                                                                             \
    if (GOAT_G2_SETPRIO) __builtin_amdgcn_s_setprio(0);                                                             \
  } while (0)

#if GOAT_G2_ROTATED
  // ---- rotated software pipeline -------------------------------------------------------------------------------
  // The single barrier of a K-tile sits at the top of its LAST k-step: by then every wave holds the tile's last fragments in
  // registers, so the stage is free one k-step before its MFMAs end.  Behind that barrier a wave (1) reads the first FD
  // k-steps of fragments of the NEXT tile, (2) issues the MFMAs of the last k-step of THIS tile, which cover the latency
  // of (1), and (3) issues the LDS-DMA of tile t+NSTAGE into the stage just freed, so that a DMA has NSTAGE-1 whole K-tiles
  // to land even in a 2-stage ring.  (The round-1 loop had its barrier between K-tiles: every wave met it with nothing
  // queued on the MFMA pipe, then waited for the first fragment reads — 400-600 of ~2900 cycles per K-tile.)
  constexpr int DSPREAD = GOAT_G2_SPREAD;      // k-steps the DMA instructions of one tile are spread over (1: all at once)
  static_assert(DSPREAD >= 1 && DSPREAD <= 3, "the DMA of a tile is issued within the three k-steps that follow the barrier");
#pragma unroll
  for (int t = 0; t < NSTAGE; ++t) GOAT_ISSUE(t);                   // every stage is free at the start
  wait_vm<(NSTAGE - 1) * LOADS>();
  __builtin_amdgcn_s_barrier();                                      // tile 0 is visible to every wave
#pragma unroll
  for (int d = 0; d < FD; ++d) {
    if (d == 0) GOAT_LOAD_FRAGS(smem_base, smem_base + TLA::BYTES, 0, 0);
    if (d == 1) GOAT_LOAD_FRAGS(smem_base, smem_base + TLA::BYTES, 1, 1);
    if (d == 2) GOAT_LOAD_FRAGS(smem_base, smem_base + TLA::BYTES, 2, 2);
  }
  static_assert(KSTEPS == 4 && FD >= 1 && FD <= 3, "k-step unrolling below is written for BK = 64");
  // DMA instruction j_ of the tile whose issue started in iteration (t_) - slot: slot 0 = right behind the barrier
#define GOAT_DMA_SLOT(slot_)                                                                                        \
  do {                                                                                                              \
    if ((slot_) < DSPREAD && ((slot_) == 0 || t > 0)) {                                                            \
      __builtin_amdgcn_sched_barrier(0);                                                                            \
      _Pragma("unroll") for (int j = 0; j < LOADS; ++j)                                                             \
        if (j * DSPREAD / LOADS == (slot_)) GOAT_ISSUE_ONE(t + NSTAGE - ((slot_) == 0 ? 0 : 1), j);               \
      __builtin_amdgcn_sched_barrier(0);                                                                            \
    }                                                                                                               \
  } while (0)
#define GOAT_KSTEP(ks_)                                                                                            \
  do {                                                                                                              \
    constexpr int left_ = (KSTEPS - (ks_) < FD ? KSTEPS - (ks_) : FD) - 1; /* later k-steps whose reads may stay in flight */ \
    wait_lgkm<(left_ * RD > 15 ? 15 : left_ * RD)>();                                                                                        \
    if ((ks_) + FD < KSTEPS) GOAT_LOAD_FRAGS(sa, sb, (ks_) + FD < KSTEPS ? (ks_) + FD : 0, (ks_) + FD < KSTEPS ? (ks_) + FD : 0); \
    GOAT_MMA(ks_);                                                                                                  \
    GOAT_DMA_SLOT((ks_) + 1);                                                                                       \
  } while (0)
#if GOAT_G2_TIMING
  uint32_t tm_wait = 0, tm_bar = 0, tm_comp = 0;
  const uint32_t tm_start = (uint32_t)__builtin_amdgcn_s_memtime();
  uint32_t tm_c = tm_start;
#endif
  for (int t = 0; t < nkt; ++t) {
    const uint32_t sa = smem_base + (t % NSTAGE) * STAGE, sb = sa + TLA::BYTES;
    const uint32_t na = smem_base + ((t + 1) % NSTAGE) * STAGE, nb = na + TLA::BYTES;
    GOAT_KSTEP(0);
    GOAT_KSTEP(1);
    GOAT_KSTEP(2);
#if GOAT_G2_TIMING
    const uint32_t tm_a = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
    wait_lgkm<0>();                                     // the last fragments of tile t are in registers: this wave is done with the stage
    wait_vm<(NSTAGE - 2) * LOADS>();                    // this wave's pieces of tile t+1 have landed
#if GOAT_G2_TIMING
    const uint32_t tm_b = (uint32_t)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    __builtin_amdgcn_s_barrier();
#if GOAT_G2_TIMING
    const uint32_t tm_c2 = (uint32_t)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    tm_comp += tm_a - tm_c; tm_wait += tm_b - tm_a; tm_bar += tm_c2 - tm_b; tm_c = tm_c2;
#endif
#pragma unroll
    for (int d = 0; d < FD; ++d) {
      if (d == 0) GOAT_LOAD_FRAGS(na, nb, 0, 0);
      if (d == 1) GOAT_LOAD_FRAGS(na, nb, 1, 1);
      if (d == 2) GOAT_LOAD_FRAGS(na, nb, 2, 2);
    }
    GOAT_MMA(3);
    GOAT_DMA_SLOT(0);      // tile t+NSTAGE -> the stage just freed (beyond the end: harmless, bounds-checked or never read)
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#undef GOAT_DMA_SLOT
#else
  // ---- round-1 loop: barrier between K-tiles ---------------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < NSTAGE - 1; ++t) GOAT_ISSUE(t);
#if GOAT_G2_TIMING
  uint32_t tm_wait = 0, tm_bar = 0, tm_comp = 0;
  const uint32_t tm_start = (uint32_t)__builtin_amdgcn_s_memtime();
  uint32_t tm_c = tm_start;
#endif
  for (int t = 0; t < nkt; ++t) {
#if GOAT_G2_TIMING
    const uint32_t tm_a = (uint32_t)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    wait_vm<(NSTAGE - 2) * LOADS>();
#if GOAT_G2_TIMING
    const uint32_t tm_b = (uint32_t)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    __builtin_amdgcn_s_barrier();
#if GOAT_G2_TIMING
    const uint32_t tm_c2 = (uint32_t)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    tm_comp += tm_a - tm_c; tm_wait += tm_b - tm_a; tm_bar += tm_c2 - tm_b; tm_c = tm_c2;
#endif
    if (!INTERLEAVE) GOAT_ISSUE(t + NSTAGE - 1);
    const uint32_t sa = smem_base + (t % NSTAGE) * STAGE;
    const uint32_t sb = sa + TLA::BYTES;
#define GOAT_KSTEP(ks_)                                                                                            \
  do {                                                                                                              \
    constexpr int left_ = (KSTEPS - (ks_) < FD ? KSTEPS - (ks_) : FD) - 1;                                          \
    wait_lgkm<(left_ * RD > 15 ? 15 : left_ * RD)>();                                                                                        \
    if ((ks_) + FD < KSTEPS) GOAT_LOAD_FRAGS(sa, sb, (ks_) + FD < KSTEPS ? (ks_) + FD : 0, (ks_) + FD < KSTEPS ? (ks_) + FD : 0); \
    GOAT_MMA(ks_);                                                                                                  \
    if (INTERLEAVE) {                                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                            \
      _Pragma("unroll") for (int j = 0; j < LOADS; ++j)                                                             \
        if (j * SPREAD / LOADS == (ks_)) GOAT_ISSUE_ONE(t + NSTAGE - 1, j);                                         \
      __builtin_amdgcn_sched_barrier(0);                                                                            \
    }                                                                                                               \
  } while (0)
#pragma unroll
    for (int d = 0; d < FD; ++d) {
      if (d == 0) GOAT_LOAD_FRAGS(sa, sb, 0, 0);
      if (d == 1) GOAT_LOAD_FRAGS(sa, sb, 1, 1);
      if (d == 2) GOAT_LOAD_FRAGS(sa, sb, 2, 2);
    }
    static_assert(KSTEPS == 4 && FD >= 1 && FD <= 3, "k-step unrolling below is written for BK = 64");
    GOAT_KSTEP(0);
    GOAT_KSTEP(1);
    GOAT_KSTEP(2);
    GOAT_KSTEP(3);
  }
#endif
#undef GOAT_MMA
  // x act' epilogues (FFN dgrad): block row 0 of the saved pre-activation is requested HERE, behind the last MFMAs and across the
  // pipeline drain; store_tile_bf16 keeps two block rows of it in flight from then on (gemm_epilogue.hpp).  Only in instantiations
  // whose accumulators leave room for two block rows; the others fetch it in place.
  constexpr bool BF16OUT = !SPLITK && sizeof(OutT) == 2;
  constexpr int AHEAD = (BF16OUT && MI * NI * 16 + 2 * Staging<NI>::CHUNKS * 4 <= 128) ? 2 : 0;
  typedef AuxAhead<NI, EPI, AHEAD> Ahead;
  Ahead ahead;
  if constexpr (Ahead::ON) load_aux_rows<Staging<NI>::CHUNKS, Staging<NI>::CPR>(p, m0 + wm * WROWS, n0 + wn * WCOLS, lane, ahead.v[0]);
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();
#undef GOAT_ISSUE
#undef GOAT_ISSUE_ONE
#undef GOAT_LOAD_FRAGS
#undef GOAT_KSTEP

  if (TA && do_colsum) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      float v = bsum[i] + __shfl_xor(bsum[i], 32, 64);
      const int row = m0 + wm * WROWS + i * 32 + l31;
      if (hi == 0 && row < p.M) atomicAdd(p.colsum + row, v);
    }
  }

#if GOAT_G2_TIMING
  if (p.aux != nullptr && lane == 0 && EPI == GOAT_EPI_NONE) {
    uint32_t* o = reinterpret_cast<uint32_t*>(p.aux) + ((size_t)blockIdx.x * NW + wave) * 4;
    o[0] = tm_wait; o[1] = tm_bar; o[2] = tm_comp; o[3] = (uint32_t)__builtin_amdgcn_s_memtime() - tm_start;
  }
#endif
  // ------------------------------------------------------------------ epilogue
  if (GOAT_G2_NOEPI) {      // keep every accumulator live (an unused one would take its MFMAs with it)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) asm volatile("" ::"v"(acc[i][j]));
    return;
  }
  const int wrow0 = wm * WROWS, wcol0 = wn * WCOLS;
  if constexpr (!BF16OUT) {
    // (patch origin: wave-uniform — `wave` went through readfirstlane, m0 / n0 come from the block id; no PIN here, see store_tile_f32)
    store_tile_f32<MI, NI, SPLITK, GOAT_G2_STORE != 0, false>(p, accs, m0 + wrow0, n0 + wcol0, lane);
  } else {
    // each wave stages through its own slice of the (now free) LDS ring
    static_assert(NW * Staging<NI>::WSLICE <= NSTAGE * STAGE, "per-wave epilogue slices must fit the LDS ring");
    store_tile_bf16<MI, NI, EPI, AHEAD, (Ahead::ON ? 1 : 0)>(p, accs, smem + wave * Staging<NI>::WSLICE, m0 + wrow0, n0 + wcol0, lane, ahead);
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <class CF, bool TA, bool TB, typename OutT, int EPI, bool SPLITK, int NSTAGE>
__global__ __launch_bounds__(CF::NTH) void gemm2_kernel(G2Args p) {
  gemm2_tile<CF, TA, TB, OutT, EPI, SPLITK, NSTAGE>(p, xcd_chunk_position(blockIdx.x, gridDim.x), blockIdx.y);
}

// Grouped weight-gradient launch: up to GROUP_MAX (24) independent TN problems (dW_i = dY_i^T · X_i, float32 out, unsplit)
// share one grid, so the many small weight gradients of a layer fill the chip together instead of each being split
// along the contraction (atomics + a zero fill) to do so.  Problem i owns tiles [tile_start[i], tile_start[i+1]).
constexpr int GROUP_MAX = 48;   // (the argument block stays under the 4 KiB kernel-argument limit)
// One problem of a grouped launch, 64 bytes: what cannot be recomputed on the device.  (Round 1-5 passed a whole G2Args — 120 bytes —
// per problem: 24 problems per launch; the text encoder's 47 weight gradients then took two launches, each with its own ramp and
// tail: 16 -> 24 problems per launch was worth 1 % of the step, profiles/round5_wgrad_group_max.txt.)
struct GroupProb {
  const void* A; const void* B; void* C; float* colsum;
  int lda, ldb, ldc;
  int M, N, Kc;
  short accum, group_m;
  int pad_;
  template <int BM, int BN>
  __host__ __device__ __forceinline__ G2Args expand() const {
    G2Args a;
    a.A = A; a.B = B; a.C = C; a.bias = nullptr; a.aux = nullptr;
    a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldaux = 0;
    a.M = M; a.N = N; a.Kc = Kc;
    a.tiles_m = (M + BM - 1) / BM;
    a.tiles_n = (N + BN - 1) / BN;
    a.k_tiles_per_split = (Kc + BK - 1) / BK;
    a.a_bytes = (uint32_t)Kc * (uint32_t)lda * 2u;      // transposed operands: Kc rows of lda / ldb elements (checked < 2 GiB on the host)
    a.b_bytes = (uint32_t)Kc * (uint32_t)ldb * 2u;
    a.colsum = colsum;
    a.accum = accum;
    a.group_m = group_m;
    return a;
  }
};
static_assert(sizeof(GroupProb) == 64, "GroupProb is 64 bytes");
static_assert(sizeof(GroupProb) * GROUP_MAX + 4 * (2 * GROUP_MAX + 8) + 32 <= 4000, "GroupArgs (and the balanced launch's iteration table) must fit the kernel-argument segment");
struct GroupArgs {
  GroupProb prob[GROUP_MAX];
  int tile_start[GROUP_MAX + 1];
  int n;
};
// the problem (of n) that owns position pos, problem i owning [start[i], start[i + 1])
__device__ __forceinline__ int group_problem_of(const int (&start)[GROUP_MAX + 1], int n, int pos) {
  int pi = 0;
#pragma unroll
  for (int i = 1; i < GROUP_MAX; ++i)
    if (i < n && pos >= start[i]) pi = i;
  return pi;
}
template <class CF, int NSTAGE>
__global__ __launch_bounds__(CF::NTH) void gemm2_group_kernel(GroupArgs g) {
  const int pos = xcd_chunk_position(blockIdx.x, gridDim.x);
  const int pi = group_problem_of(g.tile_start, g.n, pos);
  const G2Args p = g.prob[pi].template expand<CF::BM, CF::BN>();
  gemm2_tile<CF, true, true, float, GOAT_EPI_NONE, false, NSTAGE>(p, pos - g.tile_start[pi], 0);
}

// ---- host side: ONE dispatch chain for the lockstep, ping-pong and persistent main loops ------------------------------------------------
// Every refusal is decided by goat_tiles::gemm_row / grouped_row (gemm_tiles.hpp) before the chain is entered; the chain turns the accepted
// run-time values into template constants and instantiates for a tile exactly what its table row lists.  A main loop is a policy L:
// L::LOOP (its rows) and L::launch<CF, TA, TB, OutT, EPI, SPLITK, NSTAGE>, which names the kernel, its threads, LDS bytes and grid.
using goat_tiles::Row;

struct GemmCall {      // one accepted goat_gemm_bf16 launch
  hipStream_t st;
  const G2Args& a;
  int trans_a, trans_b, dtype_out, epi, split, stages;
};

template <class L, class CF>
constexpr Row row_of() { return *goat_tiles::find_row(L::LOOP, CF::BM, CF::BN, CF::EIGHT); }      // (no such row: not a constant expression)
template <class CF>
constexpr bool is_tile(const Row& r) { return r.bm == CF::BM && r.bn == CF::BN && r.eight == CF::EIGHT; }
// every table row of unit u is one of CFs: asserted beside each unit's with_tile, whose arms they are (a row without an arm would be
// accepted by the query and refused by the launch)
template <class... CFs>
constexpr bool unit_covered(goat_tiles::Unit u) {
  for (const Row& r : goat_tiles::TABLE)
    if (r.unit == u && !(is_tile<CFs>(r) || ...)) return false;
  return true;
}

// run-time ring depth -> template constant, for the depths in MASK only: f(std::integral_constant<int, NSTAGE>)
template <unsigned MASK, class F>
int with_stages(int stages, F&& f) {
  if constexpr ((MASK & goat_tiles::S2) != 0) if (stages == 2) return f(std::integral_constant<int, 2>());
  if constexpr ((MASK & goat_tiles::S3) != 0) if (stages == 3) return f(std::integral_constant<int, 3>());
  if constexpr ((MASK & goat_tiles::S4) != 0) if (stages == 4) return f(std::integral_constant<int, 4>());
  return GOAT_E_ARG;
}

// runtime epilogue id of a bf16 launch -> template constant: f(std::integral_constant<int, GOAT_EPI_...>)
template <class F>
int with_epilogue(int epi, F&& f) {
  switch (epi) {
    case GOAT_EPI_NONE: return f(std::integral_constant<int, GOAT_EPI_NONE>());
    case GOAT_EPI_GELU: return f(std::integral_constant<int, GOAT_EPI_GELU>());
    case GOAT_EPI_RELU: return f(std::integral_constant<int, GOAT_EPI_RELU>());
    case GOAT_EPI_MUL_DGELU: return f(std::integral_constant<int, GOAT_EPI_MUL_DGELU>());
    case GOAT_EPI_MUL_DRELU: return f(std::integral_constant<int, GOAT_EPI_MUL_DRELU>());
  }
  return GOAT_E_ARG;
}

template <class L, class CF, bool TA, bool TB, typename OutT, int EPI, bool SPLITK>
int launch_stages(const GemmCall& c) {
  return with_stages<row_of<L, CF>().stages>(c.stages, [&](auto ns) {
    return L::template launch<CF, TA, TB, OutT, EPI, SPLITK, decltype(ns)::value>(c.st, c.a, c.split);
  });
}

// output type, split and epilogue.  (Float32 results carry no epilogue; GOAT_EPI_ACCUM is a flag of G2Args.  Transposed A: gemm_row let only
// GOAT_EPI_NONE through.)
template <class L, class CF, bool TA, bool TB>
int dispatch2(const GemmCall& c) {
  if constexpr (row_of<L, CF>().f32) {
    if (c.split > 1) return launch_stages<L, CF, TA, TB, float, GOAT_EPI_NONE, true>(c);
    if (c.dtype_out == GOAT_F32) return launch_stages<L, CF, TA, TB, float, GOAT_EPI_NONE, false>(c);
  }
  if constexpr (TA && !L::DEAD_WGRAD_EPILOGUES) return launch_stages<L, CF, TA, TB, bf16_t, GOAT_EPI_NONE, false>(c);
  else return with_epilogue(c.epi, [&](auto e) { return launch_stages<L, CF, TA, TB, bf16_t, decltype(e)::value, false>(c); });
}

// the operand layouts of the row
template <class L, class CF>
int dispatch_layout(const GemmCall& c) {
  constexpr unsigned LAYOUTS = row_of<L, CF>().layouts;
  if constexpr ((LAYOUTS & goat_tiles::NN) != 0) if (!c.trans_a && !c.trans_b) return dispatch2<L, CF, false, false>(c);
  if constexpr ((LAYOUTS & goat_tiles::NT) != 0) if (!c.trans_a && c.trans_b) return dispatch2<L, CF, false, true>(c);
  if constexpr ((LAYOUTS & goat_tiles::TT) != 0) if (c.trans_a && c.trans_b) return dispatch2<L, CF, true, true>(c);
  return GOAT_E_ARG;
}

struct LockstepLoop {
  static constexpr goat_tiles::Loop LOOP = goat_tiles::LOCKSTEP;
  // The transposed-A tiles of this loop have always been compiled with the four activation epilogues too (56 kernels of gemm2.hip and
  // gemm3.hip that no request reaches: the old dispatch lacked an `else`).  Kept, so that the device code stays as it was; false drops them.
  static constexpr bool DEAD_WGRAD_EPILOGUES = true;
  template <class CF, bool TA, bool TB, typename OutT, int EPI, bool SPLITK, int NSTAGE>
  static int launch(hipStream_t st, const G2Args& a, int split) {
    constexpr int SMEM = smem_bytes<CF, TA, TB, NSTAGE>();
    static_assert(SMEM <= 160 * 1024, "LDS ring exceeds the CU's 160 KiB: the table row lists a ring depth its tile cannot hold");
    return launch_kernel<gemm2_kernel<CF, TA, TB, OutT, EPI, SPLITK, NSTAGE>>(dim3(a.tiles_m * a.tiles_n, SPLITK ? split : 1), dim3(CF::NTH), SMEM, st, a);
  }
};

template <class CF>
int launch_group(hipStream_t st, const GroupArgs& g, int stages) {
  return with_stages<row_of<LockstepLoop, CF>().group_stages>(stages, [&](auto ns) {
    constexpr int NSTAGE = decltype(ns)::value, SMEM = smem_bytes<CF, true, true, NSTAGE>();
    static_assert(SMEM <= 160 * 1024, "LDS ring exceeds the CU's 160 KiB");
    return launch_kernel<gemm2_group_kernel<CF, NSTAGE>>(dim3(g.tile_start[g.n]), dim3(CF::NTH), SMEM, st, g);
  });
}

}  // namespace goat_g2

// gemm3.hip: the rows of unit GEMM3
int goat_g3_gemm(const goat_g2::GemmCall& c, const goat_tiles::Row& row);
int goat_g3_group(hipStream_t st, const goat_g2::GroupArgs& g, const goat_tiles::Row& row, int stages);
