// The workgroup order the share selections write for the launches whose key loops differ in length (sta_share.hip: the sliding
// expert's row lists for vorta_attn_fwd_varlen; sta_share_all.hip: the full expert's tile lists for vorta_attn_fwd_tilelist):
// the (slot, query block) pairs by kept tile count, descending, equal counts in index order -- a counting sort (at most
// max_count + 1 distinct counts; a dead slot counts 0): every wave histograms a contiguous span of the pairs, the spans'
// histograms become start positions, every wave walks its span again and scatters.  No atomics: a pair's place is a function
// of the counts alone.  One workgroup of OW waves; each including source holds its own copy of the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sta_geometry.h"
#include "sta_rank.h"

namespace vorta_sta {

constexpr int OW = 8;  // waves of the ordering workgroup
constexpr int MAX_BINS = MAX_TILES + 1;

struct OParams {
  const int32_t* n_heads_dev; int n_heads;
  int n_tiles, n_sel, blocks_per_group;  // n_sel: the largest count
  const int32_t* sel_count;
  int32_t* order;
};

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

static __global__ __launch_bounds__(OW * 64) void sta_share_order_kernel(const OParams p) {
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

// host: the launch (one workgroup) on `st`.  static, as the kernel: each including object launches its own copy
static inline void launch_order(const int32_t* n_heads_dev, int n_heads, int n_tiles, int n_sel, int blocks_per_group,
                                const int32_t* sel_count, int32_t* order, hipStream_t st) {
  OParams o{};
  o.n_heads_dev = n_heads_dev; o.n_heads = n_heads;
  o.n_tiles = n_tiles; o.n_sel = n_sel; o.blocks_per_group = blocks_per_group;
  o.sel_count = sel_count; o.order = order;
  hipLaunchKernelGGL(sta_share_order_kernel, dim3(1), dim3(OW * 64), 0, st, o);
}

}  // namespace vorta_sta
