// Full-attention key tiles kept by MASS SHARE for gfx950: include/vorta_hip.h vorta_sta_select_tiles_share_all.
//
// vorta_sta_select_tiles_share keeps at most the WINDOW's number of key tiles and expands them into per-(slot, query tile) row
// lists.  The full-attention expert may keep up to ALL n_tiles tiles, and a row list per (slot, query tile) of that length is
// the whole sequence again for every tile (Hunyuan-129f: 150 lists of 118 896 rows per head).  So this selection stops at the
// TILE list: query tile i of head slot y keeps the fewest tiles, in the rank order of sta_rank.h (tile i first, then j != i by
// descending score, ties to the lower j, a NaN by its bits), whose scores -- the matrix sta_mass.hip left at the start of ws --
// sum to mass_share * rows_per_tile, at least 1, at most n_tiles; vorta_attn_fwd_tilelist reads key rows through the tile list
// and the one tile-major q_rows table.  Two launches:
//   sta_share_all_kernel     one workgroup per (slot, 4 query tiles), a wave per query tile: integer keys of the wave's row of
//                            the matrix in LDS, the rank, every score scattered to its rank, ONE lane sums them in rank order
//                            in fp32 (the order is the source's), the count is broadcast, sta_rank.h's ascending list straight
//                            into sel_tiles (-1 behind the count), the count and the list's length.  No row table.
//   sta_share_order_kernel   sta_order.h: the launch's workgroups by tile count, descending
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

constexpr int QB = 4;  // query tiles per selection workgroup: one per wave

struct AParams {
  const int32_t* n_heads_dev; int n_heads;
  int tok, n_tiles, t_eff;
  float threshold;      // mass_share * rows_per_tile, fp32
  const float* scores;  // [y][i][j]
  int32_t* sel_count; int32_t* sel_tiles; int32_t* kv_len;
};

__global__ __launch_bounds__(256) void sta_share_all_kernel(const AParams p) {
  __shared__ uint32_t keys[QB][MAX_TILES];
  __shared__ float ranked[QB][MAX_TILES];  // ranked[r] = the score of the tile of rank r
  __shared__ int32_t sel[QB][MAX_TILES];
  const int y = blockIdx.y;
  if (y >= p.n_heads || (p.n_heads_dev && y >= *p.n_heads_dev)) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * QB + w;
  if (i >= p.n_tiles) return;  // (no workgroup barrier below: every wave works on rows of its own)
  const float* row = p.scores + ((int64_t)y * p.n_tiles + i) * p.n_tiles;
  for (int j = lane; j < p.n_tiles; j += 64) keys[w][j] = order_key(row[j]);
  wave_sync();

  // ---- rank (sta_rank.h): a permutation of [0, n_tiles), so every score has a place ----
  for (int j = lane; j < p.n_tiles; j += 64) {
    const int rank = vorta_sta::tile_rank(keys[w], p.n_tiles, i, j);
    ranked[w][rank] = row[j];
    sel[w][j] = rank;  // (the tile's rank for now: ascending_list turns the ranks into the list)
  }
  wave_sync();

  // ---- the shortest prefix that reaches the threshold: one fp32 chain in rank order ----
  int count = p.n_tiles;
  if (lane == 0) {
    float sum = 0.f;
    for (int r = 0; r < p.n_tiles; ++r) {
      sum += ranked[w][r];
      if (sum >= p.threshold) { count = r + 1; break; }  // (a NaN sum never compares: every tile is kept)
    }
  }
  count = __shfl(count, 0);

  int32_t* sel_out = p.sel_tiles + ((int64_t)y * p.n_tiles + i) * p.n_tiles;
  vorta_sta::ascending_list(sel[w], p.n_tiles, count, sel_out);
  for (int e = count + lane; e < p.n_tiles; e += 64) sel_out[e] = -1;
  if (lane == 0) {
    p.sel_count[(int64_t)y * p.n_tiles + i] = count;
    p.kv_len[(int64_t)y * p.n_tiles + i] = count * p.tok + p.t_eff;
  }
}

// (no window: every tile is a candidate.  The geometry's other numbers are the window selections')
int geometry(const vorta_sta_share_all_args* a, Geometry& g) {
  const int32_t window[3] = {1, 1, 1};
  const int rc = vorta_sta::geometry(a->latent, a->tile, window, a->t_eff, g);
  if (rc == VORTA_OK && (int64_t)g.n_tiles * g.tok + a->t_eff > 0x7fffffff) return VORTA_EINVAL;
  return rc;
}

}  // namespace

extern "C" int vorta_sta_select_tiles_share_all_args_size(void) { return (int)sizeof(vorta_sta_share_all_args); }

extern "C" int vorta_sta_select_tiles_share_all(const vorta_sta_share_all_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_sta_share_all_args)) return VORTA_EINVAL;
  Geometry g{};
  const int rc = geometry(a, g);
  if (rc != VORTA_OK) return rc;
  if (g.n_tiles > MAX_TILES) return VORTA_EUNSUPPORTED;
  if (a->n_heads < 0 || a->n_heads > 65535) return VORTA_EINVAL;
  if (!(a->mass_share > 0.f && a->mass_share <= 1.f)) return VORTA_EINVAL;  // (a NaN fails both)
  const int r = a->rows_per_tile;
  if ((r != 8 && r != 16 && r != 32) || r > g.tok || a->blocks_per_group < 1) return VORTA_EINVAL;
  if (a->n_heads == 0) return VORTA_OK;
  if (!a->ws || ((uintptr_t)a->ws & 15) || !a->sel_count || !a->sel_tiles || !a->kv_len) return VORTA_EINVAL;
  if (((uintptr_t)a->sel_count | (uintptr_t)a->sel_tiles | (uintptr_t)a->kv_len | (uintptr_t)a->order) & 3) return VORTA_EINVAL;
  if ((int64_t)a->n_heads * g.n_tiles * a->blocks_per_group > 0x7fffffff) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  AParams s{};
  s.n_heads_dev = a->n_heads_dev; s.n_heads = a->n_heads;
  s.tok = g.tok; s.n_tiles = g.n_tiles; s.t_eff = a->t_eff;
  s.threshold = a->mass_share * (float)r;
  s.scores = a->ws; s.sel_count = a->sel_count; s.sel_tiles = a->sel_tiles; s.kv_len = a->kv_len;
  hipLaunchKernelGGL(sta_share_all_kernel, dim3((unsigned)((g.n_tiles + QB - 1) / QB), (unsigned)a->n_heads), dim3(256), 0, st,
                     s);
  if (a->order)
    vorta_sta::launch_order(a->n_heads_dev, a->n_heads, g.n_tiles, g.n_tiles, a->blocks_per_group, a->sel_count, a->order, st);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? VORTA_OK : vorta_set_hip_error(err);
}
