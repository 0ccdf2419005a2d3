// Sliding-tile geometry as row tables for gfx950: include/vorta_hip.h vorta_sta_build_tables.
//
// The reference expresses the sliding-tile expert as (1) a permutation of Q,K,V into tile-major order
// (tile.py:7-41), (2) a FlexAttention BlockMask over (S+T)^2 built from a mask_mod
// (sliding_attn_flex.py:101-134) and (3) the inverse permutation of the output (tile.py:44-78).  Here the
// same geometry becomes two int32 tables consumed by the gather attention kernel: built once per
// (geometry, t_eff) -- the moment the reference builds its BlockMask (pipeline_hunyuan.py:378-392).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace {

struct SParams {
  int lat[3], tile[3], nt[3], half[3], cnt[3];
  int S, tok, n_tiles, n_kv_video, n_kv, t_eff;
  const int32_t* row_map;
  int32_t* q_rows; int32_t* kv_rows;
};

__device__ __forceinline__ int raster_of(const SParams& p, int tt, int th, int tw, int within) {
  const int c = within % p.tile[2];
  const int b = (within / p.tile[2]) % p.tile[1];
  const int a = within / (p.tile[2] * p.tile[1]);
  return ((tt * p.tile[0] + a) * p.lat[1] + (th * p.tile[1] + b)) * p.lat[2] + (tw * p.tile[2] + c);
}

__global__ __launch_bounds__(256) void sta_q_rows_kernel(const SParams p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.S) return;
  const int ti = i / p.tok, within = i - ti * p.tok;
  const int tw = ti % p.nt[2], th = (ti / p.nt[2]) % p.nt[1], tt = ti / (p.nt[2] * p.nt[1]);
  const int r = raster_of(p, tt, th, tw, within);
  p.q_rows[i] = p.row_map ? p.row_map[r] : r;
}

__global__ __launch_bounds__(256) void sta_kv_rows_kernel(const SParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.n_tiles * p.n_kv) return;
  const int qt = (int)(i / p.n_kv);
  const int j = (int)(i - (int64_t)qt * p.n_kv);
  int r;
  if (j < p.n_kv_video) {
    const int q3[3] = {qt / (p.nt[2] * p.nt[1]), (qt / p.nt[2]) % p.nt[1], qt % p.nt[2]};
    const int slot = j / p.tok, within = j - slot * p.tok;
    const int a3[3] = {slot / (p.cnt[2] * p.cnt[1]), (slot / p.cnt[2]) % p.cnt[1], slot % p.cnt[2]};
    int kt[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      // torch.clamp(x, min=half, max=n-1-half): min first, then max (sliding_attn_flex.py:118-120)
      const int centre = min(max(q3[d], p.half[d]), p.nt[d] - 1 - p.half[d]);
      kt[d] = max(centre - p.half[d], 0) + a3[d];
    }
    r = raster_of(p, kt[0], kt[1], kt[2], within);
  } else {
    r = p.S + (j - p.n_kv_video);
  }
  p.kv_rows[i] = p.row_map ? p.row_map[r] : r;
}

int fill(const vorta_sta_args* a, SParams& p) {
  if (!a || a->struct_size != sizeof(vorta_sta_args)) return VORTA_EINVAL;
  p.S = 1; p.tok = 1; p.n_tiles = 1;
  int nkt = 1;
  for (int d = 0; d < 3; ++d) {
    if (a->latent[d] <= 0 || a->tile[d] <= 0 || a->window[d] <= 0) return VORTA_EINVAL;
    if (a->latent[d] % a->tile[d]) return VORTA_EINVAL;  // hunyuan.py:264-267 raises ValueError
    p.lat[d] = a->latent[d]; p.tile[d] = a->tile[d]; p.nt[d] = a->latent[d] / a->tile[d];
    p.half[d] = a->window[d] / 2;
    p.cnt[d] = min(p.nt[d], 2 * p.half[d] + 1);
    p.S *= p.lat[d]; p.tok *= p.tile[d]; p.n_tiles *= p.nt[d]; nkt *= p.cnt[d];
  }
  if (a->t_eff < 0) return VORTA_EINVAL;
  p.t_eff = a->t_eff;
  p.n_kv_video = nkt * p.tok;
  p.n_kv = p.n_kv_video + p.t_eff;
  p.row_map = a->row_map; p.q_rows = a->q_rows; p.kv_rows = a->kv_rows;
  return VORTA_OK;
}

__global__ __launch_bounds__(256) void seq_row_map_kernel(int32_t* out, int n, int seg_len, int seg_stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (i / seg_len) * seg_stride + i % seg_len;
}

// ---- partial geometry: a tile that does not divide the latent grid (vorta_sta_build_tables_partial) ----
// nt = ceil(latent / tile) tiles per dimension, the last one thinner.  Only the LAST tile of a dimension is thin, so every
// slab / strip / tile before a token's own is full and its tile coordinates come from three divisions.
struct PParams {
  int lat[3], tile[3], nt[3], cnt[3], nf[3];  // nf: distinct window starts of a dimension = nt - cnt + 1
  int S, n_tiles, n_lists, stride, t_eff;
  const int32_t* row_map;
  int32_t* q_rows; int32_t* kv_rows;
};

__global__ __launch_bounds__(256) void sta_partial_q_rows_kernel(const PParams p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.S) return;
  const int slab = p.tile[0] * p.lat[1] * p.lat[2];  // tokens of a full slab of tiles
  const int tt = i / slab;
  int rem = i - tt * slab;
  const int a_t = min(p.tile[0], p.lat[0] - tt * p.tile[0]);
  const int strip = a_t * p.tile[1] * p.lat[2];
  const int th = rem / strip;
  rem -= th * strip;
  const int b_t = min(p.tile[1], p.lat[1] - th * p.tile[1]);
  const int full = a_t * b_t * p.tile[2];
  const int tw = rem / full;
  const int within = rem - tw * full;
  const int c_t = min(p.tile[2], p.lat[2] - tw * p.tile[2]);
  // raster order of the tile's own (a_t, b_t, c_t) box
  const int c = within % c_t, b = (within / c_t) % b_t, a = within / (c_t * b_t);
  const int r = ((tt * p.tile[0] + a) * p.lat[1] + (th * p.tile[1] + b)) * p.lat[2] + (tw * p.tile[2] + c);
  p.q_rows[i] = p.row_map ? p.row_map[r] : r;
}

// key list l = (f0, f1, f2), the first tile of a clamped window in every dimension: the window's tiles are neighbours, so
// their union is ONE box of the grid, [f * tile, min((f + cnt) * tile, latent)) per dimension -- listed in raster order of
// that box (the softmax does not see key order), then the valid text rows; the rest of the row repeats the list's first
// entry (never read: the launch's n_kv ends before it)
__global__ __launch_bounds__(256) void sta_partial_kv_rows_kernel(const PParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.n_lists * p.stride) return;
  const int l = (int)(i / p.stride);
  int j = (int)(i - (int64_t)l * p.stride);
  const int f3[3] = {l / (p.nf[2] * p.nf[1]), (l / p.nf[2]) % p.nf[1], l % p.nf[2]};
  int lo[3], ext[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = f3[d] * p.tile[d];
    ext[d] = min((f3[d] + p.cnt[d]) * p.tile[d], p.lat[d]) - lo[d];
  }
  const int n_video = ext[0] * ext[1] * ext[2];
  if (j >= n_video + p.t_eff) j = 0;
  int r;
  if (j < n_video) {
    const int c = j % ext[2], b = (j / ext[2]) % ext[1], a = j / (ext[2] * ext[1]);
    r = ((lo[0] + a) * p.lat[1] + (lo[1] + b)) * p.lat[2] + (lo[2] + c);
  } else {
    r = p.S + (j - n_video);
  }
  p.kv_rows[i] = p.row_map ? p.row_map[r] : r;
}

int fill_partial(const vorta_sta_args* a, PParams& p, int32_t* list_n_kv) {
  if (!a || a->struct_size != sizeof(vorta_sta_args)) return VORTA_EINVAL;
  int64_t S = 1, n_lists = 1, n_tiles = 1, longest = 1;
  for (int d = 0; d < 3; ++d) {
    if (a->latent[d] <= 0 || a->tile[d] <= 0 || a->window[d] <= 0) return VORTA_EINVAL;
    p.lat[d] = a->latent[d]; p.tile[d] = a->tile[d];
    p.nt[d] = (a->latent[d] + a->tile[d] - 1) / a->tile[d];
    const int half = a->window[d] / 2;
    p.cnt[d] = min(p.nt[d], 2 * half + 1);
    p.nf[d] = p.nt[d] - p.cnt[d] + 1;
    S *= p.lat[d]; n_tiles *= p.nt[d]; n_lists *= p.nf[d];
    longest *= min(p.cnt[d] * p.tile[d], p.lat[d]);  // the window that starts at tile 0
  }
  if (a->t_eff < 0 || S + a->t_eff > 0x7fffffff || n_tiles > 0x7fffffff) return VORTA_EINVAL;
  p.S = (int)S; p.n_tiles = (int)n_tiles; p.n_lists = (int)n_lists; p.t_eff = a->t_eff;
  p.stride = (int)longest + p.t_eff;
  p.row_map = a->row_map; p.q_rows = a->q_rows; p.kv_rows = a->kv_rows;
  if (list_n_kv)
    for (int l = 0; l < p.n_lists; ++l) {
      const int f3[3] = {l / (p.nf[2] * p.nf[1]), (l / p.nf[2]) % p.nf[1], l % p.nf[2]};
      int n = 1;
      for (int d = 0; d < 3; ++d) n *= min((f3[d] + p.cnt[d]) * p.tile[d], p.lat[d]) - f3[d] * p.tile[d];
      list_n_kv[l] = n + p.t_eff;
    }
  return VORTA_OK;
}

}  // namespace

extern "C" int vorta_sta_partial_sizes(const vorta_sta_args* a, int32_t* n_tiles, int32_t* n_lists, int32_t* list_stride,
                                       int32_t* list_n_kv, int32_t list_n_kv_cap) {
  PParams p{};
  int rc = fill_partial(a, p, nullptr);
  if (rc != VORTA_OK) return rc;
  if (list_n_kv) {
    if (list_n_kv_cap < p.n_lists) return VORTA_EINVAL;
    fill_partial(a, p, list_n_kv);
  }
  if (n_tiles) *n_tiles = p.n_tiles;
  if (n_lists) *n_lists = p.n_lists;
  if (list_stride) *list_stride = p.stride;
  return VORTA_OK;
}

extern "C" int vorta_sta_build_tables_partial(const vorta_sta_args* a, void* hip_stream) {
  PParams p{};
  int rc = fill_partial(a, p, nullptr);
  if (rc != VORTA_OK) return rc;
  if (!p.q_rows || !p.kv_rows) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(sta_partial_q_rows_kernel, dim3((p.S + 255) / 256), dim3(256), 0, st, p);
  const int64_t n = (int64_t)p.n_lists * p.stride;
  if ((n + 255) / 256 > 0x7fffffff) return VORTA_EINVAL;
  hipLaunchKernelGGL(sta_partial_kv_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

extern "C" int vorta_sta_table_sizes(const vorta_sta_args* a, int32_t* n_tiles, int32_t* tok, int32_t* n_kv) {
  SParams p{};
  int rc = fill(a, p);
  if (rc != VORTA_OK) return rc;
  if (n_tiles) *n_tiles = p.n_tiles;
  if (tok) *tok = p.tok;
  if (n_kv) *n_kv = p.n_kv;
  return VORTA_OK;
}

extern "C" int vorta_sta_build_tables(const vorta_sta_args* a, void* hip_stream) {
  SParams p{};
  int rc = fill(a, p);
  if (rc != VORTA_OK) return rc;
  if (!p.q_rows || !p.kv_rows) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(sta_q_rows_kernel, dim3((p.S + 255) / 256), dim3(256), 0, st, p);
  const int64_t n = (int64_t)p.n_tiles * p.n_kv;
  if ((n + 255) / 256 > 0x7fffffff) return VORTA_EINVAL;
  hipLaunchKernelGGL(sta_kv_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

extern "C" int vorta_seq_row_map(int32_t* row_map, int32_t n_tokens, int32_t seg_len, int32_t seg_stride_rows,
                                 void* hip_stream) {
  if (!row_map || n_tokens < 0 || seg_len <= 0 || seg_stride_rows < 0) return VORTA_EINVAL;
  if (n_tokens == 0) return VORTA_OK;
  hipLaunchKernelGGL(seq_row_map_kernel, dim3((n_tokens + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream,
                     row_map, n_tokens, seg_len, seg_stride_rows);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
