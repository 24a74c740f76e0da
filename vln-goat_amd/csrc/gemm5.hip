// The ping-pong main loop (gemm5_tile.hpp) instantiated for its tile family, as itself and in its persistent form; reached through
// goat_gemm_bf16 / goat_wgrad_grouped with nstage | GOAT_GEMM_PP (nstage 2 = number of B buffers in LDS).
#include "gemm5_tile.hpp"

using namespace goat_g5;

// tile of a PINGPONG / PERSISTENT row -> type: f(CF{})
template <class F>
static int with_tile(const Row& r, F&& f) {
  if (is_tile<P256x256>(r)) return f(P256x256{});
  if (is_tile<P192x256>(r)) return f(P192x256{});
  if (is_tile<P128x256>(r)) return f(P128x256{});
  if (is_tile<P256x128>(r)) return f(P256x128{});
  if (is_tile<P128x128>(r)) return f(P128x128{});
  return GOAT_E_ARG;
}
static_assert(unit_covered<P256x256, P192x256, P128x256, P256x128, P128x128>(goat_tiles::GEMM5), "a table row of this unit has no with_tile arm");

int goat_g5_gemm(const GemmCall& c, const Row& row) {
  if (row.loop == goat_tiles::PERSISTENT) return with_tile(row, [&](auto cf) { return dispatch_layout<PersistentLoop, decltype(cf)>(c); });
  return with_tile(row, [&](auto cf) { return dispatch_layout<PingPongLoop, decltype(cf)>(c); });
}

int goat_g5_group(hipStream_t st, const GroupArgs& g, const Row& row) {
  return with_tile(row, [&](auto cf) {
    if constexpr (row_of<PingPongLoop, decltype(cf)>().group_stages != 0) return pp_launch_group<decltype(cf)>(st, g);
    return GOAT_E_ARG;
  });
}

int goat_g5_group_sk(hipStream_t st, const GroupArgs& g, const Row& row, void* ws, int64_t ws_bytes) {
  return with_tile(row, [&](auto cf) {
    if constexpr (row_of<PingPongLoop, decltype(cf)>().balanced) return pp_launch_group_sk<decltype(cf)>(st, g, ws, ws_bytes);
    return GOAT_E_ARG;
  });
}

int goat_g5_group_sk_ws_bytes(const Row& row) {
  return with_tile(row, [&](auto cf) {
    if constexpr (row_of<PingPongLoop, decltype(cf)>().balanced) return (int)pp_sk_ws_bytes<decltype(cf)>();
    return -1;
  });
}
