// Sliding-tile key tiles chosen by CONTENT for gfx950: include/vorta_hip.h vorta_sta_select_tiles.
//
// The window expert of sta_tables.hip gives query tile i the clamped window of tiles around it: a choice by position.  Here
// the same NUMBER of key tiles (n_sel = cnt_0 cnt_1 cnt_2) is chosen per head and per query tile from the data: tile i
// itself and the n_sel - 1 tiles j != i with the largest <mean q of tile i, mean k of tile j>, ties to the lower j, emitted
// in ascending j and expanded through the tile-major q_rows table into the key list the gather attention kernels read
// (kv_rows[y][i][n_kv], text rows last).  Two launches:
//   sta_tile_means_kernel     HBM bound: q and k of the selected heads are read once.  One workgroup per (tile, slot, q|k);
//                             16 lanes hold one 256-byte row as 16-byte loads, so the 256 threads hold 16 rows a pass; row
//                             ids are fetched a pass ahead of the rows they address; fp32 sums in registers, then ONE
//                             reduction over the 16 row lanes through LDS in a fixed order (the result repeats bit for bit)
//   sta_select_expand_kernel  one workgroup per (slot, 4 query tiles), a wave per query tile: the slot's k means pass through
//                             LDS in chunks of 64 tiles (a lane per key tile, rows padded to 129 floats against bank
//                             conflicts), scores in fp32 on the vector units, kept as order-preserving integer keys; then
//                             the tail of sta_rank.h, which sta_share.hip runs too: rank by counting, the ranks below n_sel
//                             as an ascending list, the tile's key list in 16-byte stores
// phases = 3 ranks a score matrix another statistic left in ws (sta_mass.hip) with the same tail: the wave's keys come from
// its row of the matrix in place of the staged means.
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

constexpr int D = 128;          // head_dim: 16 lanes x 8 elements
constexpr int ROW_LANES = 16;   // rows of a tile in flight per pass (256 threads / 16 lanes a row)
constexpr int UNR = 4;          // passes requested before the first is summed
constexpr int QB = 4;           // query tiles per selection workgroup: one per wave
constexpr int KT = 64;          // key tiles staged per chunk: one per lane
constexpr int KPAD = D + 1;     // floats per staged row
// (vorta_sta::MAX_TILES: keys and lists of a wave live in LDS: QB x MAX_TILES x (4 + 4) bytes)

struct MParams {
  const char* x[2]; int64_t sh[2], ss[2];  // q, k: byte strides
  const int32_t* head_list; const int32_t* n_heads_dev; int n_heads;
  const int32_t* q_rows;
  int tok, n_tiles;
  float* ws;  // [n_heads][2][n_tiles][D]
};

struct EParams {
  const int32_t* n_heads_dev; int n_heads;
  const int32_t* q_rows; const int32_t* row_map;
  int tok, n_tiles, n_sel, S, t_eff;
  const float* ws;
  const float* scores;  // phases 3: score[y][i][j] of another statistic (sta_mass.hip), ranked in place of <mean q, mean k>
  int32_t* sel_tiles;
  int32_t* kv_rows; int64_t kv_sh, kv_sg;
};

template <typename T> __device__ __forceinline__ float to_f(T v) { return (float)v; }

template <typename T>
__global__ __launch_bounds__(256) void sta_tile_means_kernel(const MParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  __shared__ float part[ROW_LANES][D];
  const int tile = blockIdx.x, y = blockIdx.y, which = blockIdx.z;
  if (y >= p.n_heads || (p.n_heads_dev && y >= *p.n_heads_dev)) return;  // (uniform: before any barrier)
  const int head = p.head_list ? p.head_list[y] : y;
  const int rl = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const char* xb = p.x[which] + (int64_t)head * p.sh[which] + sub * 16;
  const int64_t ss = p.ss[which];
  const int32_t* rows = p.q_rows + (int64_t)tile * p.tok;

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  int ids[UNR];
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int i = rl + ROW_LANES * u;
    ids[u] = i < p.tok ? rows[i] : 0;
  }
  for (int base = rl; base < p.tok; base += ROW_LANES * UNR) {
    V8 v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (base + ROW_LANES * u < p.tok) v[u] = *(const V8*)(xb + (int64_t)ids[u] * ss);
    // the ids of the NEXT passes leave before this pass's rows are summed
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = base + ROW_LANES * (UNR + u);
      ids[u] = i < p.tok ? rows[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (base + ROW_LANES * u < p.tok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += to_f<T>(v[u][j]);
      }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[rl][sub * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < D) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < ROW_LANES; ++r) s += part[r][threadIdx.x];  // fixed order
    p.ws[(((int64_t)y * 2 + which) * p.n_tiles + tile) * D + threadIdx.x] = s / (float)p.tok;
  }
}

__global__ __launch_bounds__(256) void sta_select_expand_kernel(const EParams p) {
  __shared__ float ks[KT][KPAD];
  __shared__ __attribute__((aligned(16))) float qs[QB][D];
  __shared__ uint32_t keys[QB][MAX_TILES];
  __shared__ int32_t sel[QB][MAX_TILES];
  const int y = blockIdx.y;
  if (y >= p.n_heads || (p.n_heads_dev && y >= *p.n_heads_dev)) return;  // (uniform: before any barrier)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * QB + w;
  const bool active = i < p.n_tiles;  // wave-uniform; an idle wave of the last workgroup still stages and meets the barriers
  const float* qbar = p.ws + ((int64_t)y * 2 + 0) * p.n_tiles * D;
  const float* kbar = p.ws + ((int64_t)y * 2 + 1) * p.n_tiles * D;
  if (p.scores) {
    // ---- scores given: the wave's row of the matrix becomes its keys (no barrier on this path) ----
    if (active)
      for (int j = lane; j < p.n_tiles; j += 64) keys[w][j] = order_key(p.scores[((int64_t)y * p.n_tiles + i) * p.n_tiles + j]);
  } else {
    for (int d = lane; d < D; d += 64) qs[w][d] = active ? qbar[(int64_t)i * D + d] : 0.f;
  }

  // ---- scores: lane = key tile of the staged chunk, d ascending ----
  for (int c0 = 0; !p.scores && c0 < p.n_tiles; c0 += KT) {
    __syncthreads();  // (the previous chunk is consumed; qs is written)
    const int n_c = min(KT, p.n_tiles - c0);
    for (int e = threadIdx.x; e < n_c * (D / 4); e += 256) {
      const int r = e / (D / 4), d4 = e % (D / 4);
      const f32x4 v = *(const f32x4*)(kbar + (int64_t)(c0 + r) * D + d4 * 4);
      ks[r][d4 * 4 + 0] = v[0]; ks[r][d4 * 4 + 1] = v[1]; ks[r][d4 * 4 + 2] = v[2]; ks[r][d4 * 4 + 3] = v[3];
    }
    __syncthreads();
    if (lane < n_c) {
      float s = 0.f;
#pragma unroll 8
      for (int d4 = 0; d4 < D / 4; ++d4) {
        const f32x4 qv = *(const f32x4*)&qs[w][d4 * 4];  // one address per wave: a broadcast
        s = fmaf(qv[0], ks[lane][d4 * 4 + 0], s);
        s = fmaf(qv[1], ks[lane][d4 * 4 + 1], s);
        s = fmaf(qv[2], ks[lane][d4 * 4 + 2], s);
        s = fmaf(qv[3], ks[lane][d4 * 4 + 3], s);
      }
      keys[w][c0 + lane] = order_key(s);
    }
  }
  if (!active) return;  // (no barrier below: every wave works on rows of its own)
  vorta_sta::wave_sync();  // (the keys are written)

  // ---- selection and expansion (sta_rank.h): tile i and the n_sel - 1 others of highest key are the ranks below n_sel ----
  for (int j = lane; j < p.n_tiles; j += 64) sel[w][j] = vorta_sta::tile_rank(keys[w], p.n_tiles, i, j);
  vorta_sta::ascending_list(sel[w], p.n_tiles, p.n_sel, p.sel_tiles + ((int64_t)y * p.n_tiles + i) * p.n_sel);
  vorta_sta::expand_key_list(p.kv_rows + (int64_t)y * p.kv_sh + (int64_t)i * p.kv_sg, sel[w], p.n_sel, p.tok, p.t_eff, p.S,
                             p.q_rows, p.row_map);
}

int geometry(const vorta_sta_select_args* a, Geometry& g) { return vorta_sta::geometry(a->latent, a->tile, a->window, a->t_eff, g); }

}  // namespace

extern "C" int vorta_sta_select_tiles_args_size(void) { return (int)sizeof(vorta_sta_select_args); }

extern "C" int64_t vorta_sta_select_tiles_ws_floats(const vorta_sta_select_args* a) {
  Geometry g{};
  if (!a || a->struct_size != sizeof(vorta_sta_select_args) || a->n_heads < 0 || geometry(a, g) != VORTA_OK) return VORTA_EINVAL;
  return (int64_t)a->n_heads * 2 * g.n_tiles * D;
}

extern "C" int vorta_sta_select_tiles(const vorta_sta_select_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_sta_select_args)) return VORTA_EINVAL;
  Geometry g{};
  int rc = geometry(a, g);
  if (rc != VORTA_OK) return rc;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != D) return VORTA_EUNSUPPORTED;
  if (g.n_tiles > MAX_TILES) return VORTA_EUNSUPPORTED;
  if (a->n_heads < 0 || a->n_heads > 65535 || a->phases < 0 || a->phases > 3) return VORTA_EINVAL;
  if (a->n_heads == 0) return VORTA_OK;
  const int n_kv = g.n_sel * g.tok + a->t_eff;
  const bool means = a->phases < 2, select = a->phases != 1;
  if (!a->q_rows || !a->ws || ((uintptr_t)a->ws & 15)) return VORTA_EINVAL;
  if (means) {
    const vorta_tensor* xs[2] = {&a->q, &a->k};
    for (const vorta_tensor* x : xs)
      if (!x->ptr || ((uintptr_t)x->ptr & 15) || (x->stride_s % 8) || (x->stride_h % 8) || x->stride_s < D) return VORTA_EINVAL;
  }
  if (select) {
    if (!a->sel_tiles) return VORTA_EINVAL;
    rc = vorta_sta::check_key_list_table(a->kv_rows, a->kv_rows_stride_h, a->kv_rows_stride_g, g.n_tiles, n_kv);
    if (rc != VORTA_OK) return rc;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  if (means) {
    MParams m{};
    const int64_t esz = 2;
    m.x[0] = (const char*)a->q.ptr; m.sh[0] = a->q.stride_h * esz; m.ss[0] = a->q.stride_s * esz;
    m.x[1] = (const char*)a->k.ptr; m.sh[1] = a->k.stride_h * esz; m.ss[1] = a->k.stride_s * esz;
    m.head_list = a->head_list; m.n_heads_dev = a->n_heads_dev; m.n_heads = a->n_heads;
    m.q_rows = a->q_rows; m.tok = g.tok; m.n_tiles = g.n_tiles; m.ws = a->ws;
    const dim3 grid((unsigned)g.n_tiles, (unsigned)a->n_heads, 2);
    if (a->dtype == VORTA_BF16)
      hipLaunchKernelGGL(sta_tile_means_kernel<__bf16>, grid, dim3(256), 0, st, m);
    else
      hipLaunchKernelGGL(sta_tile_means_kernel<_Float16>, grid, dim3(256), 0, st, m);
  }
  if (select) {
    EParams e{};
    e.n_heads_dev = a->n_heads_dev; e.n_heads = a->n_heads;
    e.q_rows = a->q_rows; e.row_map = a->row_map;
    e.tok = g.tok; e.n_tiles = g.n_tiles; e.n_sel = g.n_sel; e.S = g.S; e.t_eff = a->t_eff;
    e.ws = a->ws; e.scores = a->phases == 3 ? a->ws : nullptr; e.sel_tiles = a->sel_tiles;
    e.kv_rows = a->kv_rows; e.kv_sh = a->kv_rows_stride_h; e.kv_sg = a->kv_rows_stride_g;
    hipLaunchKernelGGL(sta_select_expand_kernel, dim3((unsigned)((g.n_tiles + QB - 1) / QB), (unsigned)a->n_heads), dim3(256),
                       0, st, e);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? VORTA_OK : vorta_set_hip_error(err);
}
