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
//                            tile count, descending, equal counts in index order -- a counting sort (at most n_sel + 1 distinct
//                            counts; a dead slot counts 0): every wave histograms a contiguous span of the pairs, the spans'
//                            histograms become start positions, every wave walks its span again and scatters.  No atomics: a
//                            pair's place is a function of the counts alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"
#include "sta_geometry.h"
#include "sta_rank.h"

namespace {
using vorta_sta::Geometry;
using vorta_sta::MAX_TILES;
using vorta_sta::order_key;
using vorta_sta::wave_sync;

constexpr int QB = 4;        // query tiles per selection workgroup: one per wave
constexpr int OW = 8;        // waves of the ordering workgroup
constexpr int MAX_BINS = MAX_TILES + 1;

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

struct OParams {
  const int32_t* n_heads_dev; int n_heads;
  int n_tiles, n_sel, blocks_per_group;
  const int32_t* sel_count;
  int32_t* order;
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

// One pass of a wave over its span [i0, i1) of the pairs, 64 a step: a pair of tile count c takes the place cnt[c] holds and
// advances it -- lanes of one count by ballot + prefix count, the counts of a step one after the other.  order = null: the
// histogram alone.
__device__ __forceinline__ void order_walk(const OParams& p, int n_live, int i0, int i1, int32_t* cnt, int32_t* order) {
  const int lane = threadIdx.x & 63;
  const int per_slot = p.n_tiles * p.blocks_per_group;
  for (int base = i0; base < i1; base += 64) {
    const int item = base + lane;
    const bool valid = item < i1;
    int c = -1;
    if (valid) {
      const int y = item / per_slot, tile = (item - y * per_slot) / p.blocks_per_group;
      c = y < n_live ? min(max(p.sel_count[(int64_t)y * p.n_tiles + tile], 0), p.n_sel) : 0;
    }
    uint64_t todo = __ballot(valid);
    while (todo) {
      const int v = __shfl(c, __ffsll((unsigned long long)todo) - 1);
      const uint64_t m = __ballot(c == v);
      if (c == v) {
        const int at = cnt[v] + __popcll(m & ((1ull << lane) - 1));
        if (order) order[at] = item;
      }
      wave_sync();
      if (lane == __ffsll((unsigned long long)m) - 1) cnt[v] += __popcll(m);
      wave_sync();
      todo &= ~m;
    }
  }
}

__global__ __launch_bounds__(OW * 64) void sta_share_order_kernel(const OParams p) {
  __shared__ int32_t cnt[OW][MAX_BINS];
  __shared__ int32_t start[MAX_BINS];
  const int w = threadIdx.x >> 6;
  const int n_bins = p.n_sel + 1;
  const int n_live = p.n_heads_dev ? min(max(*p.n_heads_dev, 0), p.n_heads) : p.n_heads;
  const int total = p.n_heads * p.n_tiles * p.blocks_per_group;
  const int span = ((total + OW - 1) / OW + 63) & ~63;
  const int i0 = min(w * span, total), i1 = min(i0 + span, total);
  for (int e = threadIdx.x; e < OW * MAX_BINS; e += OW * 64) (&cnt[0][0])[e] = 0;
  __syncthreads();
  order_walk(p, n_live, i0, i1, cnt[w], nullptr);
  __syncthreads();
  if (threadIdx.x == 0) {  // the first place of every count, longest first
    int at = 0;
    for (int v = n_bins - 1; v >= 0; --v) {
      start[v] = at;
      for (int x = 0; x < OW; ++x) at += cnt[x][v];
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < n_bins; v += OW * 64) {  // ... and of every wave's span inside it
    int at = start[v];
    for (int x = 0; x < OW; ++x) {
      const int n = cnt[x][v];
      cnt[x][v] = at;
      at += n;
    }
  }
  __syncthreads();
  order_walk(p, n_live, i0, i1, cnt[w], p.order);
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
  if (a->order) {
    OParams o{};
    o.n_heads_dev = a->n_heads_dev; o.n_heads = a->n_heads;
    o.n_tiles = g.n_tiles; o.n_sel = g.n_sel; o.blocks_per_group = a->blocks_per_group;
    o.sel_count = a->sel_count; o.order = a->order;
    hipLaunchKernelGGL(sta_share_order_kernel, dim3(1), dim3(OW * 64), 0, st, o);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? VORTA_OK : vorta_set_hip_error(err);
}
