// The 8-wave 192/256-wide tiles (and the 96-row tile) of goat_gemm_bf16 / goat_wgrad_grouped (gemm2_tile.hpp), instantiated in their
// own translation unit so that they compile in parallel with gemm2.hip.
#include "gemm2_tile.hpp"

using namespace goat_g2;

// tile of a LOCKSTEP row of this unit -> type: f(CF{})
template <class F>
static int with_tile(const Row& r, F&& f) {
  if (is_tile<T256x256>(r)) return f(T256x256{});
  if (is_tile<T192x256>(r)) return f(T192x256{});
  if (is_tile<T256x192>(r)) return f(T256x192{});
  if (is_tile<T128x256>(r)) return f(T128x256{});
  if (is_tile<T192x192>(r)) return f(T192x192{});
  if (is_tile<T96>(r)) return f(T96{});
  return GOAT_E_ARG;
}
static_assert(unit_covered<T256x256, T192x256, T256x192, T128x256, T192x192, T96>(goat_tiles::GEMM3), "a table row of this unit has no with_tile arm");

int goat_g3_gemm(const GemmCall& c, const Row& row) {
  return with_tile(row, [&](auto cf) { return dispatch_layout<LockstepLoop, decltype(cf)>(c); });
}

int goat_g3_group(hipStream_t st, const GroupArgs& g, const Row& row, int stages) {
  return with_tile(row, [&](auto cf) { return launch_group<decltype(cf)>(st, g, stages); });
}
