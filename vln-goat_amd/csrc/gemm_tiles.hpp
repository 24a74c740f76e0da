// The configurations of the bf16 GEMM family (goat_gemm_bf16, goat_wgrad_grouped, goat_wgrad_grouped_balanced) as ONE table.  Host code.
// The entry points and the two query functions (gemm2.hip) look a request up here at run time; the dispatch chain (gemm2_tile.hpp) reads the
// same row at compile time, so what is instantiated is what the table says.  The templates hold the table to what they can do: a ring
// over 160 KiB fails the static_assert of its launch, a transposed side that is not a power of two wide those of goat_g2::Tile / goat_g5::Blk,
// a row without a with_tile arm the unit_covered assert of its unit.  "4 stages only up to 128 x 128" is a choice, not a limit of the
// templates: nothing but the recorded sweep (tests/test_gemm_dispatch_table.py) guards that column.
// Adding a tile: one row here, one typedef beside its main loop, one with_tile arm in the unit that instantiates it.
#pragma once
#include "../../include/goat_hip.h"

namespace goat_tiles {

enum Loop { LOCKSTEP, PINGPONG, PERSISTENT };      // gemm2_tile.hpp; gemm5_tile.hpp: pp_tile; gemm5_tile.hpp: pp_tiles_persist
enum Unit { GEMM2, GEMM3, GEMM5 };                  // the .hip that instantiates the row's kernels (they compile in parallel)
enum : unsigned { NN = 1, NT = 2, TT = 4 };         // operand layouts (trans_a, trans_b) = (0,0) forward, (0,1) dgrad, (1,1) wgrad
constexpr unsigned S2 = 1u << 2, S3 = 1u << 3, S4 = 1u << 4;      // ring depths (ping-pong: the number of B buffers)

struct Row {
  Loop loop;
  int bm, bn;
  bool eight;             // GOAT_GEMM_8WAVES: the 128 x 128 tile on eight waves
  unsigned stages;        // ring depths.  A ring has to fit 160 KiB of LDS (3 x 64 KiB does not); 4 stages only up to 128 x 128
  unsigned layouts;       // a transposed side needs a power-of-two width (ping-pong, transposed A: a power-of-two MI = BM / 64)
  bool f32;               // float32 results: plain, GOAT_EPI_ACCUM, split_k > 1 (the persistent loop has bf16 results, unsplit)
  unsigned group_stages;  // goat_wgrad_grouped (layout TT, float32): its ring depths, 0 = not instantiated for grouped launches
  bool balanced;          // goat_wgrad_grouped_balanced
  Unit unit;
};

constexpr Row TABLE[] = {
    // loop      BM   BN   8w     stages        layouts       f32    grouped       balanced
    {LOCKSTEP, 64, 128, false, S2 | S3 | S4, NN | NT | TT, true, S2 | S3 | S4, false, GEMM2},
    {LOCKSTEP, 128, 128, false, S2 | S3 | S4, NN | NT | TT, true, S2 | S3 | S4, false, GEMM2},
    {LOCKSTEP, 128, 128, true, S2 | S3 | S4, NN | NT | TT, true, S2 | S3 | S4, false, GEMM2},
    {LOCKSTEP, 256, 128, false, S2 | S3, NN | NT | TT, true, S2 | S3, false, GEMM2},
    {LOCKSTEP, 96, 128, false, S2 | S3 | S4, NN | NT, true, 0, false, GEMM3},
    {LOCKSTEP, 128, 256, false, S2 | S3, NN | NT | TT, true, S2 | S3, false, GEMM3},
    {LOCKSTEP, 192, 256, false, S2, NN | NT, true, 0, false, GEMM3},
    {LOCKSTEP, 256, 192, false, S2, NN, true, 0, false, GEMM3},
    {LOCKSTEP, 256, 256, false, S2, NN | NT | TT, true, S2, false, GEMM3},
    {LOCKSTEP, 192, 192, false, S2 | S3, NN, true, 0, false, GEMM3},
    {PINGPONG, 256, 256, false, S2, NN | NT | TT, true, S2, true, GEMM5},
    {PINGPONG, 192, 256, false, S2, NN | NT, true, 0, false, GEMM5},
    {PINGPONG, 128, 256, false, S2, NN | NT | TT, true, S2, true, GEMM5},
    {PINGPONG, 256, 128, false, S2, NN | NT | TT, true, S2, true, GEMM5},
    {PINGPONG, 128, 128, false, S2, NN | NT | TT, true, 0, false, GEMM5},
    {PERSISTENT, 256, 256, false, S2, NN | NT, false, 0, false, GEMM5},      // K-contiguous A only
    {PERSISTENT, 192, 256, false, S2, NN | NT, false, 0, false, GEMM5},
    {PERSISTENT, 128, 256, false, S2, NN | NT, false, 0, false, GEMM5},
    {PERSISTENT, 256, 128, false, S2, NN | NT, false, 0, false, GEMM5},
    {PERSISTENT, 128, 128, false, S2, NN | NT, false, 0, false, GEMM5},
};

constexpr bool has_stage(unsigned mask, int stages) { return stages >= 2 && stages <= 4 && ((mask >> stages) & 1u); }

constexpr const Row* find_row(Loop loop, int bm, int bn, bool eight) {
  for (const Row& r : TABLE)
    if (r.loop == loop && r.bm == bm && r.bn == bn && r.eight == eight) return &r;
  return nullptr;
}

// What the `tile` (rows | columns << 16; 0 columns = 128) and `nstage` (ring depth | GOAT_GEMM_* flags) arguments of the C ABI ask for.
struct Request {
  int bm, bn, stages;
  bool eight, pp, persist;
  const Row* row() const {      // null: no such tile in this build (GOAT_GEMM_PERSIST goes with GOAT_GEMM_PP only)
    return persist && !pp ? nullptr : find_row(persist ? PERSISTENT : pp ? PINGPONG : LOCKSTEP, bm, bn, eight);
  }
};
inline Request decode_request(int tile, int nstage = 2) {
  Request q;
  q.eight = (nstage & GOAT_GEMM_8WAVES) != 0;
  q.pp = (nstage & GOAT_GEMM_PP) != 0;
  q.persist = (nstage & GOAT_GEMM_PERSIST) != 0;
  q.stages = nstage & ~(GOAT_GEMM_8WAVES | GOAT_GEMM_PP | GOAT_GEMM_PERSIST);
  q.bm = tile & 0xFFFF;
  q.bn = (tile >> 16) & 0xFFFF;
  if (q.bn == 0) q.bn = 128;
  return q;
}

// The row a goat_gemm_bf16 launch runs on, or null (GOAT_E_ARG): everything about a request that does not depend on pointers and shapes.
inline const Row* gemm_row(const Request& q, int trans_a, int trans_b, int dtype_out, int epi, int split_k) {
  const Row* r = q.row();
  if (!r || !has_stage(r->stages, q.stages)) return nullptr;
  if (!(r->layouts & (trans_a ? (trans_b ? TT : 0u) : (trans_b ? NT : NN)))) return nullptr;
  if (split_k > 1 || dtype_out == GOAT_F32 || epi == GOAT_EPI_ACCUM)       // float32 results: no epilogue but "add into C"
    return r->f32 && dtype_out == GOAT_F32 && (epi == GOAT_EPI_NONE || epi == GOAT_EPI_ACCUM) ? r : nullptr;
  if (!r->f32 && dtype_out != GOAT_BF16) return nullptr;
  // bf16 results.  Weight-gradient layout (transposed A): without an epilogue only — the activation epilogues belong to forward / dgrad,
  // and not instantiating them saves a quarter of the build.  THE place of that rule: dispatch2 instantiates accordingly.
  return epi == GOAT_EPI_NONE || (!trans_a && epi >= GOAT_EPI_GELU && epi <= GOAT_EPI_MUL_DRELU) ? r : nullptr;
}

// ... a goat_wgrad_grouped launch.  (No persistent form; the eight-wave flag goes with the lockstep 128 x 128 tile, as the table says.)
inline const Row* grouped_row(const Request& q) {
  const Row* r = q.persist ? nullptr : q.row();
  return r && has_stage(r->group_stages, q.stages) ? r : nullptr;
}

// ... a goat_wgrad_grouped_balanced launch (ping-pong tiles, two B buffers).
inline const Row* balanced_row(const Request& q) {
  const Row* r = find_row(PINGPONG, q.bm, q.bn, false);
  return r && r->balanced ? r : nullptr;
}

}  // namespace goat_tiles
