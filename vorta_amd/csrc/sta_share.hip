// Sliding-tile key tiles kept by MASS SHARE for gfx950: include/vorta_hip.h vorta_sta_select_tiles_share.
//
// vorta_sta_select_tiles keeps the window's NUMBER of key tiles, n_sel, per query tile.  Here query tile i of head slot y keeps
// the FEWEST tiles, in the same rank order (tile i first, then j != i by descending score, ties to the lower j, a NaN by its
// bits), whose scores sum to mass_share * rows_per_tile -- the stated share of the softmax mass that the sampled rows of the
// tile put on the key tiles (sta_mass.hip left score[y][i][j] at the start of ws; a row sums to rows_per_tile) -- at least 1,
// at most n_sel.  Two launches:
//   sta_share_select_kernel  one workgroup per (slot, 4 query tiles), a wave per query tile: order-preserving integer keys of
//                            the wave's row of the matrix in LDS, rank by counting, the scores of ranks < n_sel scattered to
//                            their rank, ONE lane sums them in rank order in fp32 (a serial chain: the order is the source's),
//                            the count is broadcast, then ascending list by ballot + prefix count and the key list with
//                            16-byte stores (the kept tiles' rows, then the text rows), the count and the list's length
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

namespace {
using vorta_sta::Geometry;
using vorta_sta::MAX_TILES;

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

// a float as an unsigned key of the same order (sta_select.hip: -0 first made +0; a total order, NaNs included)
__device__ __forceinline__ uint32_t order_key(float s) {
  const uint32_t b = __float_as_uint(s + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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

  // ---- rank: tile i is rank 0, a tile j != i follows the tiles of higher key and the equal ones of lower index ----
  for (int j0 = 0; j0 < p.n_tiles; j0 += 64) {
    const int j = j0 + lane;
    if (j < p.n_tiles) {
      const uint32_t mine = keys[w][j];
      int rank = 0;
      if (j != i) {
        rank = 1;
        for (int o = 0; o < p.n_tiles; ++o) {
          const uint32_t other = keys[w][o];  // a broadcast
          rank += (o != i && (other > mine || (other == mine && o < j))) ? 1 : 0;
        }
      }
      if (rank < p.n_sel) ranked[w][rank] = row[j];
      sel[w][j] = rank;  // (the tile's rank for now; the list overwrites entries below the ones it still reads)
    }
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

  // ---- ascending list by ballot + prefix count; unused entries -1 ----
  int32_t* sel_out = p.sel_tiles + ((int64_t)y * p.n_tiles + i) * p.n_sel;
  int n_out = 0;
  for (int j0 = 0; j0 < p.n_tiles; j0 += 64) {
    const int j = j0 + lane;
    const bool take = j < p.n_tiles && sel[w][j] < count;
    const uint64_t m = __ballot(take);
    wave_sync();  // every lane has read its rank before the list is written over the ranks of lower tiles
    if (take) {
      const int pos = n_out + __popcll(m & ((1ull << lane) - 1));  // pos <= j: below every rank still to be read
      sel[w][pos] = j;
      sel_out[pos] = j;
    }
    n_out += __popcll(m);
  }
  for (int e = count + lane; e < p.n_sel; e += 64) sel_out[e] = -1;
  wave_sync();

  // ---- expansion: entry e < count tok is q_rows[sel[e / tok] tok + e % tok], then the text rows; 4 entries a lane, one
  // 16-byte store.  Entries between the length and the next multiple of 4 repeat entry 0; none is written behind that
  const int n_vid = count * p.tok, n_kv = n_vid + p.t_eff;
  int32_t* dst = p.kv_rows + (int64_t)y * p.kv_sh + (int64_t)i * p.kv_sg;
  const int first = p.q_rows[(int64_t)sel[w][0] * p.tok];
  for (int e0 = lane * 4; e0 < n_kv; e0 += 64 * 4) {
    int t = e0 / p.tok, within = e0 - t * p.tok;
    u32x4 out;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u;
      int r = first;
      if (e < n_vid) {
        r = p.q_rows[(int64_t)sel[w][t] * p.tok + within];
      } else if (e < n_kv) {
        const int x = p.S + (e - n_vid);
        r = p.row_map ? p.row_map[x] : x;
      }
      out[u] = (uint32_t)r;
      if (++within == p.tok) { within = 0; ++t; }
    }
    *(u32x4*)(dst + e0) = out;
  }
  if (lane == 0) {
    p.sel_count[(int64_t)y * p.n_tiles + i] = count;
    p.kv_len[(int64_t)y * p.n_tiles + i] = n_kv;
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
  if (!a->q_rows || !a->ws || ((uintptr_t)a->ws & 15) || !a->sel_count || !a->sel_tiles || !a->kv_len || !a->kv_rows ||
      ((uintptr_t)a->kv_rows & 15))
    return VORTA_EINVAL;
  // 16-byte stores: both strides in whole groups of 4 entries, a tile's row long enough for its longest list rounded up to 4
  if ((a->kv_rows_stride_g % 4) || (a->kv_rows_stride_h % 4) || a->kv_rows_stride_g < n_kv ||
      a->kv_rows_stride_h < (int64_t)g.n_tiles * a->kv_rows_stride_g)
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
