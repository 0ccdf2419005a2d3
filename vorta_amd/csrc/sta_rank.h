// The tail the sliding-tile selections share (sta_select.hip: a fixed number of key tiles; sta_share.hip: the fewest for a
// mass share): a wave ranks the key tiles of its query tile from order-preserving keys in LDS, lists the tiles it keeps in
// ascending order and expands that list into the key list the gather attention kernels read.  One rank, so "share ranks as
// vorta_sta_select_tiles" (include/vorta_hip.h) holds by construction: fixed count is rank < n_sel, share is rank < count.
// Every function is called by all 64 lanes of a wave that owns the LDS rows it is given.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace vorta_sta {

// a float as an unsigned key of the same order (-0 first made +0: the two compare equal, so they must tie); a total order,
// NaNs included (a NaN by its bits), so a query tile keeps EXACTLY the number of tiles asked for whatever the data holds
__device__ __forceinline__ uint32_t order_key(float s) {
  const uint32_t b = __float_as_uint(s + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the wave's LDS writes so far are visible to its other lanes
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rank of key tile j for query tile i, by counting over keys[n_tiles]: tile i is rank 0, a tile j != i follows it, the tiles
// of higher key and the equal ones of lower index
__device__ __forceinline__ int tile_rank(const uint32_t* keys, int n_tiles, int i, int j) {
  if (j == i) return 0;
  const uint32_t mine = keys[j];
  int rank = 1;
  for (int o = 0; o < n_tiles; ++o) {
    const uint32_t other = keys[o];  // a broadcast
    rank += (o != i && (other > mine || (other == mine && o < j))) ? 1 : 0;
  }
  return rank;
}

// list[j] holds the rank of tile j on entry; on return list[0 .. count) and out[0 .. count) hold the tiles of rank < count in
// ascending order -- ballot + prefix count, 64 tiles a pass.  The list is written over the ranks: a tile's place is the number
// of kept tiles below it, pos <= j, and a pass writes only after every lane has read its rank, so no rank still to be read
// (this pass's, or a later pass's at j >= 64 passes) is overwritten.  (pos < count always: the order is total, so exactly
// `count` tiles have a rank below it.)
__device__ __forceinline__ void ascending_list(int32_t* list, int n_tiles, int count, int32_t* out) {
  const int lane = threadIdx.x & 63;
  int n_out = 0;
  for (int j0 = 0; j0 < n_tiles; j0 += 64) {
    const int j = j0 + lane;
    const bool take = j < n_tiles && list[j] < count;
    const uint64_t m = __ballot(take);
    wave_sync();
    if (take) {
      const int pos = n_out + __popcll(m & ((1ull << lane) - 1));
      if (pos < count) {
        list[pos] = j;
        out[pos] = j;
      }
    }
    n_out += __popcll(m);
  }
  wave_sync();
}

// The key list of `count` kept tiles sel[] (LDS, ascending): entry e < count tok is q_rows[sel[e / tok] tok + e % tok], then
// the t_eff text rows S, S + 1, ... (through row_map where given); 4 entries a lane, one 16-byte store (dst 16-byte aligned).
// Entries between the length and the next multiple of 4 repeat entry 0; none is written behind that.
__device__ __forceinline__ void expand_key_list(int32_t* dst, const int32_t* sel, int count, int tok, int t_eff, int S,
                                                const int32_t* q_rows, const int32_t* row_map) {
  const int lane = threadIdx.x & 63;
  const int n_vid = count * tok, n_kv = n_vid + t_eff;
  const int first = n_vid ? q_rows[(int64_t)sel[0] * tok] : 0;
  for (int e0 = lane * 4; e0 < n_kv; e0 += 64 * 4) {
    int t = e0 / tok, within = e0 - t * tok;
    u32x4 out;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u;
      int r = first;
      if (e < n_vid) {
        r = q_rows[(int64_t)sel[t] * tok + within];
      } else if (e < n_kv) {
        const int x = S + (e - n_vid);
        r = row_map ? row_map[x] : x;
      }
      out[u] = (uint32_t)r;
      if (++within == tok) { within = 0; ++t; }
    }
    *(u32x4*)(dst + e0) = out;
  }
}

// host: the kv_rows table both entry points write with 16-byte stores -- aligned, both strides in whole groups of 4 entries,
// a tile's row long enough for its longest list (n_kv entries, rounded up to 4 by the stride), a slot's rows for n_tiles tiles
inline int check_key_list_table(const int32_t* kv_rows, int64_t stride_h, int64_t stride_g, int n_tiles, int n_kv) {
  if (!kv_rows || ((uintptr_t)kv_rows & 15)) return VORTA_EINVAL;
  if ((stride_g % 4) || (stride_h % 4) || stride_g < n_kv || stride_h < (int64_t)n_tiles * stride_g) return VORTA_EINVAL;
  return VORTA_OK;
}

}  // namespace vorta_sta
