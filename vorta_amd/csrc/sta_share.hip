// Sliding-tile key tiles kept by MASS SHARE for gfx950: include/vorta_hip.h vorta_sta_select_tiles_share.
//
// vorta_sta_select_tiles keeps the window's NUMBER of key tiles, n_sel, per query tile.  Here query tile i of head slot y keeps
// the FEWEST tiles, in the same rank order (tile i first, then j != i by descending score, ties to the lower j, a NaN by its
// bits), whose scores sum to mass_share * rows_per_tile -- the stated share of the softmax mass that the sampled rows of the
// tile put on the key tiles (sta_mass.hip left score[y][i][j] at the start of ws; a row sums to rows_per_tile) -- at least 1,
// at most n_sel.  Two launches:
//   sta_share_select_kernel  one workgroup per (slot, 4 query tiles), a wave per query tile: order-preserving integer keys of
//                            the wave's row of the matrix in LDS, the rank of sta_rank.h (the one sta_select.hip keeps
//                            n_sel tiles by), the scores of ranks < n_sel scattered to their rank, ONE lane sums them in rank
//                            order in fp32 (a serial chain: the order is the source's), the count is broadcast, then
//                            sta_rank.h's ascending list and key list (the kept tiles' rows, then the text rows; 16-byte
//                            stores), the count and the list's length
//   sta_share_order_kernel   one workgroup: `order`, the (slot, query block) pairs of the variable-length attention launch by
//                            tile count, descending, equal counts in index order -- the counting sort of sta_order.h, which
//                            sta_share_all.hip runs over its own counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"
#include "sta_geometry.h"
#include "sta_rank.h"
#include "sta_order.h"

namespace {
using vorta_sta::Geometry;
using vorta_sta::MAX_TILES;
using vorta_sta::order_key;
using vorta_sta::wave_sync;

constexpr int QB = 4;        // query tiles per selection workgroup: one per wave

struct SParams {
  const int32_t* n_heads_dev; int n_heads;
  const int32_t* q_rows; const int32_t* row_map;
  int tok, n_tiles, n_sel, S, t_eff;
  float threshold;      // mass_share * rows_per_tile, fp32
  const float* scores;  // [y][i][j]
  int32_t* sel_count; int32_t* sel_tiles;
  int32_t* kv_rows; int64_t kv_sh, kv_sg;
  int32_t* kv_len;
};

__global__ __launch_bounds__(256) void sta_share_select_kernel(const SParams p) {
  __shared__ uint32_t keys[QB][MAX_TILES];
  __shared__ float ranked[QB][MAX_TILES];  // ranked[r] = the score of the tile of rank r, r < n_sel
  __shared__ int32_t sel[QB][MAX_TILES];
  const int y = blockIdx.y;
  if (y >= p.n_heads || (p.n_heads_dev && y >= *p.n_heads_dev)) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * QB + w;
  if (i >= p.n_tiles) return;  // (no workgroup barrier below: every wave works on rows of its own)
  const float* row = p.scores + ((int64_t)y * p.n_tiles + i) * p.n_tiles;
  for (int j = lane; j < p.n_tiles; j += 64) keys[w][j] = order_key(row[j]);
  wave_sync();

  // ---- rank (sta_rank.h), the scores of the ranks below n_sel scattered to their rank ----
  for (int j = lane; j < p.n_tiles; j += 64) {
    const int rank = vorta_sta::tile_rank(keys[w], p.n_tiles, i, j);
    if (rank < p.n_sel) ranked[w][rank] = row[j];
    sel[w][j] = rank;  // (the tile's rank for now: ascending_list turns the ranks into the list)
  }
  wave_sync();

  // ---- the shortest prefix that reaches the threshold: one fp32 chain in rank order ----
  int count = p.n_sel;
  if (lane == 0) {
    float sum = 0.f;
    for (int r = 0; r < p.n_sel; ++r) {
      sum += ranked[w][r];
      if (sum >= p.threshold) { count = r + 1; break; }  // (a NaN sum never compares: the count stays n_sel)
    }
  }
  count = __shfl(count, 0);

  // ---- the ranks below count as an ascending list (unused entries -1), expanded into the key list (sta_rank.h) ----
  int32_t* sel_out = p.sel_tiles + ((int64_t)y * p.n_tiles + i) * p.n_sel;
  vorta_sta::ascending_list(sel[w], p.n_tiles, count, sel_out);
  for (int e = count + lane; e < p.n_sel; e += 64) sel_out[e] = -1;
  vorta_sta::expand_key_list(p.kv_rows + (int64_t)y * p.kv_sh + (int64_t)i * p.kv_sg, sel[w], count, p.tok, p.t_eff, p.S,
                             p.q_rows, p.row_map);
  if (lane == 0) {
    p.sel_count[(int64_t)y * p.n_tiles + i] = count;
    p.kv_len[(int64_t)y * p.n_tiles + i] = count * p.tok + p.t_eff;
  }
}

int geometry(const vorta_sta_share_args* a, Geometry& g) { return vorta_sta::geometry(a->latent, a->tile, a->window, a->t_eff, g); }

}  // namespace

extern "C" int vorta_sta_select_tiles_share_args_size(void) { return (int)sizeof(vorta_sta_share_args); }

extern "C" int64_t vorta_sta_select_tiles_share_ws_floats(const vorta_sta_share_args* a) {
  Geometry g{};
  if (!a || a->struct_size != sizeof(vorta_sta_share_args) || a->n_heads < 0 || geometry(a, g) != VORTA_OK) return VORTA_EINVAL;
  return (int64_t)a->n_heads * g.n_tiles * g.n_tiles;  // the score matrices it reads
}

extern "C" int vorta_sta_select_tiles_share(const vorta_sta_share_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_sta_share_args)) return VORTA_EINVAL;
  Geometry g{};
  const int rc = geometry(a, g);
  if (rc != VORTA_OK) return rc;
  if (g.n_tiles > MAX_TILES) return VORTA_EUNSUPPORTED;
  if (a->n_heads < 0 || a->n_heads > 65535) return VORTA_EINVAL;
  if (!(a->mass_share > 0.f && a->mass_share <= 1.f)) return VORTA_EINVAL;  // (a NaN fails both)
  const int r = a->rows_per_tile;
  if ((r != 8 && r != 16 && r != 32) || r > g.tok || a->blocks_per_group < 1) return VORTA_EINVAL;
  if (a->n_heads == 0) return VORTA_OK;
  const int n_kv = g.n_sel * g.tok + a->t_eff;
  if (!a->q_rows || !a->ws || ((uintptr_t)a->ws & 15) || !a->sel_count || !a->sel_tiles || !a->kv_len) return VORTA_EINVAL;
  if (vorta_sta::check_key_list_table(a->kv_rows, a->kv_rows_stride_h, a->kv_rows_stride_g, g.n_tiles, n_kv) != VORTA_OK)
    return VORTA_EINVAL;
  if ((int64_t)a->n_heads * g.n_tiles * a->blocks_per_group > 0x7fffffff) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  SParams s{};
  s.n_heads_dev = a->n_heads_dev; s.n_heads = a->n_heads;
  s.q_rows = a->q_rows; s.row_map = a->row_map;
  s.tok = g.tok; s.n_tiles = g.n_tiles; s.n_sel = g.n_sel; s.S = g.S; s.t_eff = a->t_eff;
  s.threshold = a->mass_share * (float)r;
  s.scores = a->ws; s.sel_count = a->sel_count; s.sel_tiles = a->sel_tiles;
  s.kv_rows = a->kv_rows; s.kv_sh = a->kv_rows_stride_h; s.kv_sg = a->kv_rows_stride_g; s.kv_len = a->kv_len;
  hipLaunchKernelGGL(sta_share_select_kernel, dim3((unsigned)((g.n_tiles + QB - 1) / QB), (unsigned)a->n_heads), dim3(256), 0,
                     st, s);
  if (a->order)
    vorta_sta::launch_order(a->n_heads_dev, a->n_heads, g.n_tiles, g.n_sel, a->blocks_per_group, a->sel_count, a->order, st);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? VORTA_OK : vorta_set_hip_error(err);
}
