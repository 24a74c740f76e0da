// goat_gemm_bf16 / goat_wgrad_grouped: C entry points, tile-order choice, and the instantiations of the 4-wave and
// 128-column tiles.  The tile code itself is gemm2_tile.hpp; the 8-wave 192/256-wide tiles are instantiated in gemm3.hip.
#include "gemm5_tile.hpp"

using namespace goat_g2;

// Tile-order parameter: the group height that minimises the operand bytes the eight per-XCD L2s have to fetch,
// sum over XCDs of (distinct tile rows * BM + distinct tile columns * BN) under the kernel's own blockIdx -> tile map
// (XCD x owns one contiguous chunk of the grouped order).  Brute force once per (tiles_m, tiles_n, bm, bn), then cached.
static int pick_group_m(int tiles_m, int tiles_n, int bm, int bn) {
  if (const char* e = getenv("GOAT_GEMM_GROUP_M")) {
    int g = atoi(e);
    return g < 1 ? 1 : (g > tiles_m ? tiles_m : g);
  }
  static std::mutex mu;
  static std::unordered_map<uint64_t, int> cache;
  const uint64_t key = ((uint64_t)tiles_m << 44) | ((uint64_t)tiles_n << 24) | ((uint64_t)bm << 12) | (uint64_t)bn;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  const int nwg = tiles_m * tiles_n, q = nwg >> 3, r = nwg & 7;
  int best = 1;
  double best_cost = 1e300;
  std::vector<char> seen_m(tiles_m), seen_n(tiles_n);
  const int gmax = tiles_m < 64 ? tiles_m : 64;
  for (int gm = 1; gm <= gmax; ++gm) {
    double cost = 0;
    int pos = 0;
    for (int x = 0; x < 8; ++x) {
      const int cnt = x < r ? q + 1 : q;
      std::fill(seen_m.begin(), seen_m.end(), 0);
      std::fill(seen_n.begin(), seen_n.end(), 0);
      int dm = 0, dn = 0;
      for (int i = 0; i < cnt; ++i, ++pos) {
        const int gsz = gm * tiles_n, grp = pos / gsz, gi = pos - grp * gsz;
        const int h = std::min(tiles_m - grp * gm, gm);
        const int tn = gi / h, tm = grp * gm + (gi - tn * h);
        if (!seen_m[tm]) { seen_m[tm] = 1; ++dm; }
        if (!seen_n[tn]) { seen_n[tn] = 1; ++dn; }
      }
      cost += (double)dm * bm + (double)dn * bn;
    }
    if (cost < best_cost - 1e-9) { best_cost = cost; best = gm; }
  }
  std::lock_guard<std::mutex> lk(mu);
  cache[key] = best;
  return best;
}


// tile of a LOCKSTEP row of this unit -> type: f(CF{}).  (The other rows: gemm3.hip, gemm5.hip.)
template <class F>
static int with_tile(const Row& r, F&& f) {
  if (is_tile<T64>(r)) return f(T64{});
  if (is_tile<T256>(r)) return f(T256{});
  if (is_tile<T128X8>(r)) return f(T128X8{});
  if (is_tile<T128>(r)) return f(T128{});
  return GOAT_E_ARG;
}
static_assert(unit_covered<T64, T256, T128X8, T128>(goat_tiles::GEMM2), "a table row of this unit has no with_tile arm");

// Would goat_gemm_bf16 / goat_wgrad_grouped take this configuration?  0 or GOAT_E_ARG: the very lookup the two perform before they launch.
// No pointers, no device.
extern "C" int goat_gemm_bf16_query(int trans_a, int trans_b, int dtype_out, int epilogue, int split_k, int tile, int nstage) {
  return goat_tiles::gemm_row(goat_tiles::decode_request(tile, nstage), trans_a, trans_b, dtype_out, epilogue, split_k) ? 0 : GOAT_E_ARG;
}
extern "C" int goat_wgrad_grouped_query(int tile, int nstage) {
  return goat_tiles::grouped_row(goat_tiles::decode_request(tile, nstage)) ? 0 : GOAT_E_ARG;
}

extern "C" int goat_gemm_bf16(void* stream, int trans_a, int trans_b, int dtype_out,
                              const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                              int M, int N, int Kc, const float* bias, int epilogue,
                              void* aux, int64_t ldaux, int split_k, int tile, int nstage, float* colsum) {
  if (!A || !B || !C) return GOAT_E_ARG;
  if (colsum && !trans_a) return GOAT_E_ARG;
  if (M <= 0 || N <= 0 || Kc <= 0) return GOAT_E_SHAPE;
  if ((lda % 8) || (ldb % 8)) return GOAT_E_SHAPE;
  if ((reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(B) & 15)) return GOAT_E_SHAPE;
  // contraction tails: transposed operands are zero-filled by the bounds check; K-contiguous operands need
  // whole 64-wide tiles (callers route other shapes to goat_gemm_nt)
  if ((!trans_a || !trans_b) && (Kc % BK)) return GOAT_E_SHAPE;
  // C = (A·B) * act'(aux): no bias.  The shared epilogue (gemm_epilogue.hpp: store_tile_bf16) relies on this rejection — it reads no bias
  // in its x act' instantiations, for any main loop.
  if ((epilogue == GOAT_EPI_MUL_DGELU || epilogue == GOAT_EPI_MUL_DRELU) && (!aux || bias)) return GOAT_E_ARG;
  if ((epilogue == GOAT_EPI_ACCUM || split_k > 1) && bias) return GOAT_E_ARG;      // (both add into a float32 C)
  const goat_tiles::Request q = goat_tiles::decode_request(tile, nstage);
  const Row* row = goat_tiles::gemm_row(q, trans_a, trans_b, dtype_out, epilogue, split_k);
  if (!row) return GOAT_E_ARG;
  const int bm = row->bm, bn = row->bn;
  const int64_t a_rows = trans_a ? Kc : M, b_rows = trans_b ? Kc : N;
  const int64_t a_bytes = a_rows * lda * 2, b_bytes = b_rows * ldb * 2;
  if (a_bytes >= (1ll << 31) || b_bytes >= (1ll << 31)) return GOAT_E_SHAPE;

  G2Args a;
  a.A = A; a.B = B; a.C = C; a.bias = bias; a.aux = aux;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldaux = ldaux;
  a.M = M; a.N = N; a.Kc = Kc;
  a.tiles_m = (M + bm - 1) / bm;
  a.tiles_n = (N + bn - 1) / bn;
  a.a_bytes = (uint32_t)a_bytes; a.b_bytes = (uint32_t)b_bytes;
  a.colsum = colsum;
  a.accum = epilogue == GOAT_EPI_ACCUM;
  a.group_m = pick_group_m(a.tiles_m, a.tiles_n, bm, bn);
  const int kt = (Kc + BK - 1) / BK;
  const bool adds_into_c = split_k > 1;        // the contract of a split launch, whatever the clamp below leaves of it
  if (split_k < 1) split_k = 1;
  if (split_k > kt) split_k = kt;
  // A contraction of one K-tile leaves nothing to split: the launch runs unsplit, and must still ADD into C (it used to overwrite C:
  // tests/test_gemm_family_gpu.py, Kc = 64 with split_k 2 / 3 onto a base).  float32 C without bias was checked above.
  if (adds_into_c && split_k == 1) a.accum = 1;
  a.k_tiles_per_split = (kt + split_k - 1) / split_k;
  const GemmCall c = {ST(stream), a, trans_a, trans_b, dtype_out, epilogue, split_k, q.stages};
  if (row->unit == goat_tiles::GEMM5) return goat_g5_gemm(c, *row);
  if (row->unit == goat_tiles::GEMM3) return goat_g3_gemm(c, *row);
  return with_tile(*row, [&](auto cf) { return dispatch_layout<LockstepLoop, decltype(cf)>(c); });
}

// argument block of a grouped launch from the caller's problem list (validation shared by the two entry points)
static int build_group(const goat_wgrad_problem* probs, int n, int bm, int bn, GroupArgs& g) {
  g.n = n;
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    const goat_wgrad_problem& q = probs[i];
    if (!q.dy || !q.x || !q.dw) return GOAT_E_ARG;
    if (q.rows <= 0 || q.n_out <= 0 || q.n_in <= 0) return GOAT_E_SHAPE;
    if ((q.ld_dy % 8) || (q.ld_x % 8)) return GOAT_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(q.dy) & 15) || (reinterpret_cast<uintptr_t>(q.x) & 15)) return GOAT_E_SHAPE;
    const int64_t a_bytes = (int64_t)q.rows * q.ld_dy * 2, b_bytes = (int64_t)q.rows * q.ld_x * 2;
    if (a_bytes >= (1ll << 31) || b_bytes >= (1ll << 31)) return GOAT_E_SHAPE;
    if (q.ld_dy >= (1ll << 31) || q.ld_x >= (1ll << 31) || q.ld_dw >= (1ll << 31)) return GOAT_E_SHAPE;
    GroupProb& a = g.prob[i];
    a.A = q.dy; a.B = q.x; a.C = q.dw; a.colsum = q.dbias;
    a.lda = (int)q.ld_dy; a.ldb = (int)q.ld_x; a.ldc = (int)q.ld_dw;
    a.M = q.n_out; a.N = q.n_in; a.Kc = q.rows;
    a.accum = q.accumulate ? 1 : 0;
    const int tiles_m = (q.n_out + bm - 1) / bm, tiles_n = (q.n_in + bn - 1) / bn;
    a.group_m = (short)pick_group_m(tiles_m, tiles_n, bm, bn);
    a.pad_ = 0;
    g.tile_start[i] = tiles;
    tiles += tiles_m * tiles_n;
  }
  for (int i = n; i <= GROUP_MAX; ++i) g.tile_start[i] = tiles;
  return 0;
}

extern "C" int goat_wgrad_grouped(void* stream, const goat_wgrad_problem* probs, int n, int tile, int nstage) {
  if (!probs || n < 1 || n > GROUP_MAX) return GOAT_E_ARG;
  const goat_tiles::Request q = goat_tiles::decode_request(tile, nstage);
  const Row* row = goat_tiles::grouped_row(q);
  if (!row) return GOAT_E_ARG;
  GroupArgs g;
  if (int e = build_group(probs, n, row->bm, row->bn, g)) return e;
  if (row->unit == goat_tiles::GEMM5) return goat_g5_group(ST(stream), g, *row);
  if (row->unit == goat_tiles::GEMM3) return goat_g3_group(ST(stream), g, *row, q.stages);
  return with_tile(*row, [&](auto cf) { return launch_group<decltype(cf)>(ST(stream), g, q.stages); });
}

// Contraction-balanced form of the grouped launch (gemm5_tile.hpp: pp_group_sk_kernel): ping-pong tiles 256x256 / 128x256 / 256x128.
extern "C" int goat_wgrad_grouped_balanced(void* stream, const goat_wgrad_problem* probs, int n, int tile, void* workspace, int64_t workspace_bytes) {
  if (!probs || n < 1 || n > GROUP_MAX) return GOAT_E_ARG;
  const Row* row = goat_tiles::balanced_row(goat_tiles::decode_request(tile));
  if (!row) return GOAT_E_ARG;
  GroupArgs g;
  if (int e = build_group(probs, n, row->bm, row->bn, g)) return e;
  return goat_g5_group_sk(ST(stream), g, *row, workspace, workspace_bytes);
}

extern "C" int goat_wgrad_balanced_ws_bytes(int tile) {
  const Row* row = goat_tiles::balanced_row(goat_tiles::decode_request(tile));
  return row ? goat_g5_group_sk_ws_bytes(*row) : -1;
}
