// Gather flash-attention forward whose query groups have key lists of DIFFERENT lengths, for gfx950 (MI355X, CDNA4):
// include/vorta_hip.h vorta_attn_fwd_varlen.  16 bits (bf16 / fp16), D = 128, a kv_rows table required.
//
// vorta_attn_fwd walks one n_kv per launch.  Here group g of head slot y attends the first kv_len[y][g] entries of its list
// and nothing behind them: the sliding-tile expert under sliding_keys="share" keeps a different number of key tiles per
// (head, query tile) (sta_share.hip), and a workgroup's key loop is as long as its own list.
//
// The body (attn_varlen_body.h: attn_fwd_tilelist.hip runs it too, with key row ids from tile lists in the place of TableRows
// below) is built on the two shared ends of attn_common.h (decode_work, write_rows) and on the family's 32x32x16 scheme:
//   * swapped product S^T[kv][q] = K . Q^T: a lane owns one query and 16 + 16 of a block's 64 scores; the accumulator is the
//     B operand of O^T[d][q] = V^T . P^T as it stands;
//   * Q pre-multiplied by scale log2(e) and re-rounded, the score MFMAs seeded with minus the row's reference point, the
//     reference moved only when a row outgrows it by more than `defer` binades: the arithmetic of attn_pipe_dma_body;
//   * K tile with the 16-way XOR swizzle, V tile with the 64-byte-quadrant swizzle read through ds_read_b64_tr_b16; both
//     staged global -> LDS by DMA (the swizzle applied on the source side), rings of 2, 64-key blocks, ONE barrier a block.
// What is new:
//   * the group's length is a scalar: one load through a workgroup-uniform address, in readfirstlane form, clamped into
//     [1, n_kv].  It bounds the key loop and every row-id fetch (positions are clamped to len - 1, so no entry behind the
//     length is read and a tail block's spare rows are copies of the last listed key);
//   * a tail block (len not a multiple of 64) is masked as the table body masks it: -inf into the scores past len;
//   * the logical workgroup comes through `order` (physical block b computes order[b]): key loops of one launch differ by up
//     to n_sel x, and a grid dealt in index order ends with whichever long loops came last.  sta_share.hip writes the order
//     longest first.  NULL: the XCD-aware index order of the family.  (attn_common.h varlen_workgroup; the tables and the
//     host checks of vorta_attn_varlen_ext are its VarTables / fill_var_tables, shared with attn_fwd_i8_varlen.hip.)
// The step is simpler than attn_pipe_dma_body's: scores, softmax and P V of block j in step j (no scores one block ahead),
// K(j+1) and V(j+1) requested at the top of step j into the slots step j-1 read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"
#include "attn_varlen_body.h"

namespace {
using namespace vorta_attn;

struct ParamsVar {
  Params p;
  VarTables t;
};

// attn_varlen_body's key rows (attn_varlen_body.h): position e of the group's list is kv_rows[e]
template <int NW>
struct TableRows {
  static constexpr int CH = varlen_pieces<NW>;
  static constexpr int LDS_BYTES = 0;
  const int32_t* kv_rows;
  int len, wave, lane;
  __device__ __forceinline__ TableRows(const ParamsVar& pp, const Params& p, const Work& w, char*, int wave_, int lane_)
      : kv_rows(p.kv_rows + (int64_t)w.y * p.kv_rows_sh + (int64_t)w.grp * p.kv_rows_sg),
        len(max(1, min(__builtin_amdgcn_readfirstlane(pp.t.kv_len[(int64_t)w.y * pp.t.kv_len_sh + w.grp]), w.n_kv))),
        wave(wave_), lane(lane_) {}
  __device__ __forceinline__ void fetch(int blk, int (&rowN)[CH]) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) rowN[i] = kv_rows[min(blk * KVB + 4 * (CH * wave + i) + (lane >> 4), len - 1)];
  }
};

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_varlen_kernel(const ParamsVar pp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  __shared__ __attribute__((aligned(16))) char smem[2 * NSV * TILE_BYTES];
  attn_varlen_body<T, NW, TableRows<NW>>(pp, smem, varlen_workgroup(pp.t, pp.p));
#endif
}

template <typename T>
int launch(const ParamsVar& pp, int block_rows, hipStream_t st) {
  return launch_varlen(attn_varlen_kernel<T, 8>, attn_varlen_kernel<T, 4>, pp.p, pp, block_rows, st);
}

}  // namespace

extern "C" int vorta_attn_varlen_ext_size(void) { return (int)sizeof(vorta_attn_varlen_ext); }

extern "C" int vorta_attn_fwd_varlen(const vorta_attn_args* a, const vorta_attn_varlen_ext* ext, void* hip_stream) {
  if (!varlen_ext_sized(ext)) return VORTA_EINVAL;
  ParamsVar pp{};
  int block_rows = 0;
  int rc = fill_params(a, pp.p, block_rows, 2);  // (a dtype other than bf16 / fp16: VORTA_EUNSUPPORTED there)
  if (rc == VORTA_OK) rc = fill_var_tables(a, ext, pp.p, pp.t);  // (one body: the LDS-DMA one)
  if (rc != VORTA_OK) return rc;
  if (pp.p.n_heads == 0 || pp.p.n_groups == 0) return VORTA_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  return a->dtype == VORTA_BF16 ? launch<__bf16>(pp, block_rows, st) : launch<_Float16>(pp, block_rows, st);
}
