// Sliding-tile key tiles ranked by SAMPLED ATTENTION MASS for gfx950: include/vorta_hip.h vorta_sta_tile_mass.
//
// The statistic: r sampled query rows stand for a query tile; every sampled row x is scored against EVERY video key of its
// head, and score[i][j] = sum over the sampled rows x of tile i of the share p_x(j) of x's softmax mass that falls on key
// tile j.  vorta_sta_select_tiles(phases = 3) ranks that matrix and writes the key lists.  Two launches:
//   sta_tile_mass_kernel    the matrix pipe: a Q K^T-only flash loop, no V, no output.  Grid (key span, block of 256 sampled
//                           rows, head slot), 8 waves.  A wave owns 32 sampled rows (32 / r query tiles) and keeps their
//                           32 x 128 fragments in 32 registers for the whole launch, as the operand that puts ONE query in
//                           a lane column (S^T = K Q^T on v_mfma_f32_32x32x16): the 16 scores a lane holds of a 32-key block
//                           belong to one query, so the row max and sum are in-lane plus one half-wave exchange.  The
//                           workgroup walks its span of key tiles one tile at a time, 64 key rows (two 32-key blocks) a
//                           chunk: the rows are gathered through q_rows into LDS once per workgroup -- global -> registers a
//                           chunk ahead, row ids a chunk ahead of that, LDS double buffered, one barrier a chunk -- in the
//                           forward loop's K layout (16-way XOR swizzle of the 16-byte chunks, ds_read_b128 fragments, which
//                           are conflict free; K is the row-major operand here and wants no transposing read).  A tile's
//                           last chunk is masked to -inf past the tile's rows, so a block never holds keys of two tiles.
//                           Per (sampled row, key tile) the wave keeps a running (max, sum of exp2) in the log2 domain and
//                           writes the pair when the tile ends; it never rescales ACROSS tiles, which is what lets the key
//                           range be cut into spans with no merge between workgroups
//   sta_mass_reduce_kernel  HBM bound: a wave per (slot, query tile) reads the r x n_tiles pairs, takes each row's global
//                           max, forms p_x(j) and sums the r rows in ascending order.  No atomics: the same inputs give the
//                           same scores bit for bit
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"
#include "attn_common.h"
#include "sta_geometry.h"

namespace {
using vorta_attn::MF;
using vorta_attn::half_max;
using vorta_attn::half_sum;
using vorta_sta::Geometry;
using vorta_sta::MAX_TILES;

constexpr int D = 128;
constexpr int ROWB = D * 2;              // bytes of a key row
constexpr int NW = 8;                    // waves of a mass workgroup
constexpr int NT = NW * 64;
constexpr int XB = NW * 32;              // sampled rows of a workgroup
constexpr int KC = 64;                   // key rows staged per chunk: two 32-key blocks
constexpr int CHUNK_BYTES = KC * ROWB;   // 16 KiB; two buffers
constexpr int CH = (KC * 16) / NT;       // 16-byte pieces of a chunk per thread
constexpr int ROWSTEP = NT / 16;         // rows between a thread's pieces
constexpr int TARGET_WG = 512;           // two rounds of the 256 CUs
constexpr int RQ = 4;                    // query tiles of a reduce workgroup: one per wave
constexpr int RU = MAX_TILES / 64;       // key tiles a reduce lane holds

struct TParams {
  const char* q; const char* k;
  int64_t q_sh, q_ss, k_sh, k_ss;  // bytes
  const int32_t* head_list; const int32_t* n_heads_dev;
  const int32_t* q_rows;
  int tok, n_tiles, r, n_x, span_tiles;
  float scale_log2;
  float* pairs;  // [slot][n_x][n_tiles][2]: (max, sum of exp2 above it), log2 domain
};

struct RParams {
  const int32_t* n_heads_dev;
  int n_tiles, r, n_x;
  const float* pairs;
  float* scores;  // [slot][n_tiles][n_tiles]
};

template <typename T>
__global__ __launch_bounds__(NT, 4) void sta_tile_mass_kernel(const TParams p) {
  using V8 = typename MF<T>::v8;
  __shared__ __attribute__((aligned(16))) char smem[2 * CHUNK_BYTES];
  const int y = blockIdx.z;
  if (p.n_heads_dev && y >= *p.n_heads_dev) return;  // (uniform: before any barrier)
  const int head = p.head_list ? p.head_list[y] : y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int t0 = blockIdx.x * p.span_tiles, t1 = min(t0 + p.span_tiles, p.n_tiles);
  const int cpt = (p.tok + KC - 1) / KC;  // chunks of a key tile
  const int n_chunks = (t1 - t0) * cpt;

  // ---- the wave's sampled rows: x = i r + s stands at tile-major position i tok + floor((2 s + 1) tok / (2 r)) ----
  const int x0 = blockIdx.y * XB + wave * 32;
  const bool wave_active = x0 < p.n_x;  // an idle wave of the last block still stages and meets the barriers
  const int x = x0 + r32;
  const bool x_ok = x < p.n_x;          // a spare column repeats the last sampled row and is never written
  V8 qf[8];
  {
    const int xc = min(x, p.n_x - 1);
    const int i = xc / p.r, s = xc - i * p.r;
    const int64_t row = p.q_rows[(int64_t)i * p.tok + ((2 * s + 1) * p.tok) / (2 * p.r)];
    const char* qp = p.q + (int64_t)head * p.q_sh + row * p.q_ss + hh * 16;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const V8*)(qp + ks * 32);
  }

  // ---- loader: thread -> piece (tid & 15) of rows (tid >> 4) + 32 i of the chunk ----
  const char* kbase = p.k + (int64_t)head * p.k_sh + (tid & 15) * 16;
  const int lrow0 = tid >> 4, lcc = tid & 15;
  int k_wr[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int row = lrow0 + i * ROWSTEP;
    k_wr[i] = row * ROWB + ((lcc ^ (row & 15)) << 4);
  }
  u32x4 kreg[CH];
  int nrow[CH];
  // (rows past the tile's end repeat its last row: valid addresses, masked below)
#define FETCH_ROWS(c_)                                                                           \
  {                                                                                              \
    const int t_ = t0 + (c_) / cpt, cc_ = (c_) % cpt;                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_)                                            \
        nrow[i_] = p.q_rows[(int64_t)t_ * p.tok + min(cc_ * KC + lrow0 + i_ * ROWSTEP, p.tok - 1)]; \
  }
#define ISSUE_LOADS() \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) kreg[i_] = *(const u32x4*)(kbase + (int64_t)nrow[i_] * p.k_ss);
#define WRITE_LDS(buf_) \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) *(u32x4*)(smem + (buf_) * CHUNK_BYTES + k_wr[i_]) = kreg[i_];

  // fragment ks of the lane's key row: piece (2 ks + hh) ^ (row & 15) = 2 ks ^ (hh ^ (row & 15)), one XOR per read
  const int k_rd0 = r32 * ROWB, k_sw = (hh ^ (r32 & 15)) << 4;
#define K_RD(ks_) (k_rd0 + (k_sw ^ ((ks_) << 5)))

  if (n_chunks > 0) {
    FETCH_ROWS(0);
    ISSUE_LOADS();
    if (1 < n_chunks) { FETCH_ROWS(1); }
    WRITE_LDS(0);
    if (1 < n_chunks) { ISSUE_LOADS(); }
    if (2 < n_chunks) { FETCH_ROWS(2); }
    __syncthreads();
  }

  const float c = p.scale_log2;
  float m_run = -1e30f, l_run = 0.f;  // of the CURRENT key tile; l_run: this lane's half of the row's keys
  int tile = t0, cc = 0;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const char* sb = smem + (ch & 1) * CHUNK_BYTES;
    if (wave_active) {
      const int kv0 = cc * KC;
      const bool two = kv0 + 32 < p.tok;  // (uniform) the chunk's second 32-key block holds keys of the tile
      f32x16 s0, s1;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s0[i] = 0.f; s1[i] = -INFINITY; }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) s0 = MF<T>::mfma(*(const V8*)(sb + K_RD(ks)), qf[ks], s0);
      if (two) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s1[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) s1 = MF<T>::mfma(*(const V8*)(sb + K_RD(ks) + 32 * ROWB), qf[ks], s1);
      }
      if (kv0 + KC > p.tok) {  // the tile's last chunk: rows past the tile are -inf
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
          if (kv0 + row >= p.tok) s0[i] = -INFINITY;
          if (kv0 + 32 + row >= p.tok) s1[i] = -INFINITY;
        }
      }
      float mx = s0[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s0[i]);
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s1[i]);
      const float m_new = fmaxf(m_run, half_max(mx));
      l_run *= __builtin_amdgcn_exp2f((m_run - m_new) * c);  // (the tile's first chunk: l_run is 0)
      m_run = m_new;
      const float mc = m_run * c;
      float lsum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        lsum += __builtin_amdgcn_exp2f(fmaf(s0[i], c, -mc)) + __builtin_amdgcn_exp2f(fmaf(s1[i], c, -mc));
      l_run += lsum;
      if (cc == cpt - 1) {  // the tile ends: its pair leaves, the next tile starts from nothing (no rescale across tiles)
        const float l_tot = half_sum(l_run);
        if (x_ok && hh == 0)
          *(float2*)(p.pairs + (((int64_t)y * p.n_x + x) * p.n_tiles + tile) * 2) = make_float2(mc, l_tot);
        m_run = -1e30f;
        l_run = 0.f;
      }
    }
    if (++cc == cpt) { cc = 0; ++tile; }
    // ---- stage the next chunk (its loads were issued a chunk ago) ----
    if (ch + 1 < n_chunks) {
      WRITE_LDS((ch + 1) & 1);
      if (ch + 2 < n_chunks) { ISSUE_LOADS(); }
      if (ch + 3 < n_chunks) { FETCH_ROWS(ch + 3); }
    }
    __syncthreads();
  }
#undef FETCH_ROWS
#undef ISSUE_LOADS
#undef WRITE_LDS
#undef K_RD
}

__global__ __launch_bounds__(RQ * 64) void sta_mass_reduce_kernel(const RParams p) {
  const int y = blockIdx.y;
  if (p.n_heads_dev && y >= *p.n_heads_dev) return;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * RQ + (threadIdx.x >> 6);
  if (i >= p.n_tiles) return;  // (no barrier in this kernel: every wave works on a query tile of its own)
  const int nu = (p.n_tiles + 63) / 64;
  float acc[RU];
#pragma unroll
  for (int u = 0; u < RU; ++u) acc[u] = 0.f;
  for (int s = 0; s < p.r; ++s) {  // fixed order: s ascending
    const float2* row = (const float2*)p.pairs + ((int64_t)y * p.n_x + (int64_t)i * p.r + s) * p.n_tiles;
    float2 v[RU];
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int j = lane + 64 * u;
      v[u] = (u < nu && j < p.n_tiles) ? row[j] : make_float2(-INFINITY, 0.f);
      m = fmaxf(m, v[u].x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float l = 0.f;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      v[u].y = u < nu ? v[u].y * __builtin_amdgcn_exp2f(v[u].x - m) : 0.f;  // tile j's mass above the row's max
      l += v[u].y;
    }
    // (a butterfly: both partners add the same two values, so every lane holds the same sum, the same on every run)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off);
#pragma unroll
    for (int u = 0; u < RU; ++u) acc[u] += v[u].y / l;
  }
  float* out = p.scores + ((int64_t)y * p.n_tiles + i) * p.n_tiles;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int j = lane + 64 * u;
    if (u < nu && j < p.n_tiles) out[j] = acc[u];
  }
}

int64_t align4(int64_t n) { return (n + 3) & ~(int64_t)3; }

int check(const vorta_sta_mass_args* a, Geometry& g) {
  if (!a || a->struct_size != sizeof(vorta_sta_mass_args)) return VORTA_EINVAL;
  const int rc = vorta_sta::geometry(a->latent, a->tile, a->window, a->t_eff, g);
  if (rc != VORTA_OK) return rc;
  const int r = a->rows_per_tile;
  if ((r != 8 && r != 16 && r != 32) || r > g.tok) return VORTA_EINVAL;
  if (a->n_heads < 0 || a->n_heads > 65535) return VORTA_EINVAL;
  return VORTA_OK;
}

}  // namespace

extern "C" int vorta_sta_tile_mass_args_size(void) { return (int)sizeof(vorta_sta_mass_args); }

extern "C" int64_t vorta_sta_tile_mass_ws_floats(const vorta_sta_mass_args* a) {
  Geometry g{};
  if (check(a, g) != VORTA_OK) return VORTA_EINVAL;
  const int64_t n = g.n_tiles;
  return align4((int64_t)a->n_heads * n * n) + (int64_t)a->n_heads * n * a->rows_per_tile * n * 2;
}

extern "C" int vorta_sta_tile_mass(const vorta_sta_mass_args* a, void* hip_stream) {
  Geometry g{};
  const int rc = check(a, g);
  if (rc != VORTA_OK) return rc;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != D) return VORTA_EUNSUPPORTED;
  if (g.n_tiles > MAX_TILES) return VORTA_EUNSUPPORTED;
  if (!(a->scale > 0.f) || !(a->scale < INFINITY)) return VORTA_EINVAL;
  if (a->n_heads == 0) return VORTA_OK;
  if (!a->q_rows || !a->ws || ((uintptr_t)a->ws & 15)) return VORTA_EINVAL;
  const vorta_tensor* xs[2] = {&a->q, &a->k};
  for (const vorta_tensor* x : xs)
    if (!x->ptr || ((uintptr_t)x->ptr & 15) || (x->stride_s % 8) || (x->stride_h % 8) || x->stride_s < D) return VORTA_EINVAL;

  const int r = a->rows_per_tile;
  const int n_x = g.n_tiles * r;
  const int x_blocks = (n_x + XB - 1) / XB;
  // key spans: enough workgroups for two rounds of the chip, a span never shorter than one key tile
  int n_span = (int)((TARGET_WG + (int64_t)x_blocks * a->n_heads - 1) / ((int64_t)x_blocks * a->n_heads));
  n_span = max(1, min(n_span, g.n_tiles));
  const int span_tiles = (g.n_tiles + n_span - 1) / n_span;
  n_span = (g.n_tiles + span_tiles - 1) / span_tiles;

  TParams t{};
  t.q = (const char*)a->q.ptr; t.q_sh = a->q.stride_h * 2; t.q_ss = a->q.stride_s * 2;
  t.k = (const char*)a->k.ptr; t.k_sh = a->k.stride_h * 2; t.k_ss = a->k.stride_s * 2;
  t.head_list = a->head_list; t.n_heads_dev = a->n_heads_dev; t.q_rows = a->q_rows;
  t.tok = g.tok; t.n_tiles = g.n_tiles; t.r = r; t.n_x = n_x; t.span_tiles = span_tiles;
  t.scale_log2 = a->scale * 1.44269504088896340736f;
  t.pairs = a->ws + align4((int64_t)a->n_heads * g.n_tiles * g.n_tiles);
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)n_span, (unsigned)x_blocks, (unsigned)a->n_heads);
  if (a->dtype == VORTA_BF16)
    hipLaunchKernelGGL(sta_tile_mass_kernel<__bf16>, grid, dim3(NT), 0, st, t);
  else
    hipLaunchKernelGGL(sta_tile_mass_kernel<_Float16>, grid, dim3(NT), 0, st, t);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return vorta_set_hip_error(err);

  RParams e{};
  e.n_heads_dev = a->n_heads_dev; e.n_tiles = g.n_tiles; e.r = r; e.n_x = n_x; e.pairs = t.pairs; e.scores = a->ws;
  hipLaunchKernelGGL(sta_mass_reduce_kernel, dim3((unsigned)((g.n_tiles + RQ - 1) / RQ), (unsigned)a->n_heads), dim3(RQ * 64),
                     0, st, e);
  err = hipGetLastError();
  return err == hipSuccess ? VORTA_OK : vorta_set_hip_error(err);
}
