// Gather flash-attention forward whose query groups walk TILE lists of different lengths, for gfx950 (MI355X, CDNA4):
// include/vorta_hip.h vorta_attn_fwd_tilelist.  16 bits (bf16 / fp16), D = 128.
//
// The full-attention expert under full_keys="share" keeps, per (head, query tile), the fewest key tiles holding a share of the
// sampled softmax mass -- up to ALL n_tiles (sta_share_all.hip).  Expanded into rows, as vorta_attn_fwd_varlen wants its lists,
// that is the whole sequence per (head, query tile): 150 x 118 896 ints per head at Hunyuan-129f, 570 MB for 8 heads, written
// and read again every call.  The tile list is 150 ints.  So the key loop here reads a key row id through two levels: the
// group's tile list, then the one tile-major row table every list shares (vorta_sta_build_tables' q_rows, 475 KB, L2-resident).
//
// The body is attn_varlen_body (attn_varlen_body.h) with its row-id fetch exchanged (TileRows below); the length, the `order`
// permutation, the tail-block masking and the arithmetic are vorta_attn_fwd_varlen's, so equal lists give equal bits.
//   * the group's tile list lives in LDS, 4 KiB behind the K and V rings (68 KiB a workgroup, two workgroups a CU): the
//     workgroup copies its `count` entries once, clamped into [0, n_tiles) and pre-multiplied by tok, so a lane's lookup is one
//     ds_read_b32 and one add.  (Scalar loads would do for a uniform index; here the 16 row groups of a wave index different
//     tiles whenever a block straddles a tile edge.)
//   * tok is no multiple of the 64-key block (792 at Hunyuan, 24 in the tests), so a block straddles tiles.  A lane carries, for
//     each of its CH DMA pieces, (tile index, offset within the tile) of its position in the next block to fetch, and steps
//     them by (64 / tok, 64 % tok) with one conditional wrap: two scalar constants a workgroup, no division in the loop.
//   * the fetch runs a block ahead of the DMA request, where ROWS_OF stood; positions at or behind the length take the list's
//     LAST row (the clamp of the table launch: a tail block's spare rows are copies of the last listed key), computed once.
//   * nothing is requested behind the list's last block: the loop bound is the group's own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"
#include "attn_varlen_body.h"

namespace {
using namespace vorta_attn;

constexpr int MAX_LIST = 1024;  // tiles of a list: the limit of the selections (sta_geometry.h MAX_TILES)

struct TileTables {
  int tok, n_tiles, S, t_eff;
  const int32_t* tile_rows;
  const int32_t* tiles; int64_t tiles_sh;
  const int32_t* count; int64_t count_sh;
};

struct ParamsTl {
  Params p;
  VarTables t;  // (order alone: the lengths come from the counts)
  TileTables x;
};

template <int NW>
struct TileRows {
  static constexpr int CH = varlen_pieces<NW>;
  static constexpr int LDS_BYTES = MAX_LIST * 4;
  const int32_t* tile_rows;
  const int32_t* list;  // LDS: the first row-table index of every listed tile
  int len, n_vid, tok, S, last_row;
  int dt, dw;      // a block's 64 positions in whole tiles and rows of a tile
  int e0;          // the position of the lane's piece 0 in the next block to fetch
  int t[CH], w[CH];

  __device__ __forceinline__ TileRows(const ParamsTl& pp, const Params&, const Work& wk, char* lds, int wave, int lane) {
    const TileTables& x = pp.x;
#define UNI(v_) __builtin_amdgcn_readfirstlane(v_)
    const int count = max(1, min(UNI(x.count[(int64_t)wk.y * x.count_sh + wk.grp]), x.n_tiles));
    const int32_t* tl = x.tiles + (int64_t)wk.y * x.tiles_sh + (int64_t)wk.grp * x.n_tiles;
    tile_rows = x.tile_rows;
    tok = x.tok; S = x.S;
    n_vid = count * tok;
    len = n_vid + x.t_eff;
    int32_t* l = (int32_t*)lds;
    for (int e = threadIdx.x; e < count; e += NW * 64) l[e] = min(max(tl[e], 0), x.n_tiles - 1) * tok;
    list = l;
    if (x.t_eff > 0) {
      last_row = S + x.t_eff - 1;
    } else {
      last_row = UNI(tile_rows[min(max(UNI(tl[count - 1]), 0), x.n_tiles - 1) * tok + tok - 1]);
    }
#undef UNI
    dt = KVB / tok; dw = KVB - dt * tok;
    e0 = 4 * CH * wave + (lane >> 4);
#pragma unroll
    for (int i = 0; i < CH; ++i) {  // the one division of a lane's walk (positions below 64)
      t[i] = (e0 + 4 * i) / tok;
      w[i] = (e0 + 4 * i) - t[i] * tok;
    }
    __syncthreads();  // the list is in LDS for every wave
  }

  // (blk: the body asks for blocks 0, 1, 2, ... in order; the walk carries the position itself)
  __device__ __forceinline__ void fetch(int, int (&rowN)[CH]) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int e = e0 + 4 * i;
      int r = last_row;
      if (e < n_vid) {
        r = tile_rows[list[t[i]] + w[i]];
      } else if (e < len) {
        r = S + (e - n_vid);
      }
      rowN[i] = r;
      t[i] += dt; w[i] += dw;
      if (w[i] >= tok) { w[i] -= tok; ++t[i]; }
    }
    e0 += KVB;
  }
};

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_tilelist_kernel(const ParamsTl pp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  __shared__ __attribute__((aligned(16))) char smem[2 * NSV * TILE_BYTES + TileRows<NW>::LDS_BYTES];
  attn_varlen_body<T, NW, TileRows<NW>>(pp, smem, varlen_workgroup(pp.t, pp.p));
#endif
}

template <typename T>
int launch(const ParamsTl& pp, int block_rows, hipStream_t st) {
  return launch_varlen(attn_tilelist_kernel<T, 8>, attn_tilelist_kernel<T, 4>, pp.p, pp, block_rows, st);
}

}  // namespace

extern "C" int vorta_attn_tilelist_ext_size(void) { return (int)sizeof(vorta_attn_tilelist_ext); }

extern "C" int vorta_attn_fwd_tilelist(const vorta_attn_args* a, const vorta_attn_tilelist_ext* ext, void* hip_stream) {
  if (!ext || ext->struct_size != sizeof(vorta_attn_tilelist_ext)) return VORTA_EINVAL;
  ParamsTl pp{};
  int block_rows = 0;
  const int rc = fill_params(a, pp.p, block_rows, 2);  // (a dtype other than bf16 / fp16: VORTA_EUNSUPPORTED there)
  if (rc != VORTA_OK) return rc;
  const Params& p = pp.p;
  if (p.n_heads == 0 || p.n_groups == 0) return VORTA_OK;
  // one body (not the plain variant 1), no split keys (the lengths differ per group), no duplicate rows, host lengths
  if (a->variant == 1 || a->n_splits != 1 || a->dup_rows || a->n_kv_dev) return VORTA_EUNSUPPORTED;
  if (ext->tok < 1 || ext->n_tiles < 1 || ext->t_eff < 0 || ext->S < 0) return VORTA_EINVAL;
  if (ext->n_tiles > MAX_LIST) return VORTA_EUNSUPPORTED;
  if (a->kv_rows || (int64_t)ext->n_tiles * ext->tok + ext->t_eff != a->n_kv) return VORTA_EINVAL;
  if (!ext->tile_rows || !ext->tiles || !ext->count) return VORTA_EINVAL;
  if (((uintptr_t)ext->tile_rows | (uintptr_t)ext->tiles | (uintptr_t)ext->count | (uintptr_t)ext->order) & 3) return VORTA_EINVAL;
  // (with a q_block_table the number of lists is the caller's: the strides are checked against q_group_len's groups only)
  const int64_t lists = a->q_block_table ? 1 : p.n_groups;
  if (ext->count_stride_h < lists || ext->tiles_stride_h < lists * ext->n_tiles) return VORTA_EINVAL;
  pp.t.order = ext->order;
  pp.x.tok = ext->tok; pp.x.n_tiles = ext->n_tiles; pp.x.S = ext->S; pp.x.t_eff = ext->t_eff;
  pp.x.tile_rows = ext->tile_rows; pp.x.tiles = ext->tiles; pp.x.tiles_sh = ext->tiles_stride_h;
  pp.x.count = ext->count; pp.x.count_sh = ext->count_stride_h;
  hipStream_t st = (hipStream_t)hip_stream;
  return a->dtype == VORTA_BF16 ? launch<__bf16>(pp, block_rows, st) : launch<_Float16>(pp, block_rows, st);
}
