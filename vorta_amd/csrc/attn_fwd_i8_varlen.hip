// Int8-score gather flash-attention forward whose query groups have key lists of DIFFERENT lengths, for gfx950 (MI355X,
// CDNA4): include/vorta_hip.h vorta_attn_fwd_varlen_i8.  Operands of vorta_attn_fwd_i8 (16-bit q and out, int8 k, e4m3 v, the
// quantiser's k_bias / q_prep / k_head_scale / v_descale), tables of vorta_attn_fwd_varlen (kv_rows required, kv_len, order).
//
// Why: the sliding-tile expert under sliding_keys="share" keeps a different number of key tiles per (head, query tile)
// (sta_share.hip) and a workgroup's key loop is as long as its own list; under VORTA_ATTENTION_PRECISION=i8pv the other
// experts of the layer run the int8-score kernel, and this is that kernel walking such lists.
//
// The body IS attn_i8_body (attn_i8_body.h, VARLEN = true), step for step: the wave's own query scale, the seeded int32
// accumulators read as floats, one multiply-add into the byte domain, MX block exponents on the P V MFMA, row sums from the
// ones tile, the two roles of a SIMD's wave pair, K three blocks ahead of its read, V one, the bias tile four, rings of four,
// one wait and one barrier per two key blocks.  A launch over a list of length L therefore writes the bits vorta_attn_fwd_i8
// writes over the same list with n_kv = L (tests/test_hip_attn_varlen_i8.py holds it to that).  What differs is how the loop is
// entered and left, because a "share" list is short -- one key tile plus the text rows: 14 blocks at Hunyuan-129f, one or two
// at the test geometry -- and the fixed-length body's ends cost about three steps' time:
//   * the length is a scalar (one load through a workgroup-uniform address, readfirstlane, clamped into [1, n_kv]); it bounds
//     the loop, the tail mask and the clamp of every row-id fetch, so no list entry behind it is read and the spare rows of
//     a tail block are copies of the last listed key;
//   * only tiles of blocks the list has are requested: a list of nblk blocks asks for min(nblk, 3) K tiles, one V tile and
//     min(nblk, 4) bias tiles in the prologue, and step j asks for K(j+3), V(j+1), bias(j+4) only where they exist -- a scalar
//     compare and branch in front of each request.  (The fixed-length body asks for copies of the last key instead: 3 K, 1 V
//     and 4 bias tiles + step 0's 2 + 1 for a list of ONE block.)  The ring slots, their period of 4 and the exits of the
//     4-way unrolled loop are the parent's for every nblk mod 4: a skipped request leaves a slot stale, and a stale slot is
//     read only into the scores of a block past the end, which feed no P V;
//   * the logical workgroup comes through `order` (sta_share.hip writes the longest key loops first), clamped into the grid;
//     NULL: the family's XCD-aware index order.  (attn_common.h varlen_workgroup; the tables and the host checks of
//     vorta_attn_varlen_ext are its VarTables / fill_var_tables, shared with attn_fwd_varlen.hip.)
// Two further entries for short lists were built and taken out again, both for registers (the loop runs at the VGPR budget):
// a list of one block going from block 0's scores straight to the drain (no step 0, one barrier instead of three) spilled
// 21-38 VGPRs, 88-156 B of scratch, with the drain shared or with a drain of its own; the query conversion moved behind the
// prologue's tile requests (to run under their round trip) changed the fixed-length kernels' register allocation when written
// once for both forms.  A list of one block therefore still pays the parent's step 0 and drain.
// Resources as compiled (tests/test_build_resources_varlen_i8.py): the parent's LDS -- 4 + 4 tiles of 8 KiB, 4 bias tiles of
// 256 B, 8 x 2 seed slots of 256 B = 70 656 B <= 80 KiB, so __launch_bounds__(NW * 64, 2) keeps two workgroups on a CU -- 240
// VGPRs, no scratch, no vector spills.  The length, the block count and the two table pointers are scalar values the
// fixed-length kernels do not hold, and those run at 98-104 of 106 SGPRs: here the allocator parks scalar values in VGPR
// lanes (v_writelane / v_readlane, 2-7 a step).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"
#include "attn_i8_body.h"

namespace {
using namespace vorta_attn;

struct ParamsI8Var {
  ParamsI8 pi;
  VarTables t;
};

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_i8_varlen_kernel(const ParamsI8Var pv) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  __shared__ __attribute__((aligned(16))) char smem[SMEM_I8];
  attn_i8_body<T, NW, true, NSI8, true>(pv.pi, smem, varlen_workgroup(pv.t, pv.pi.p), pv.t.kv_len, pv.t.kv_len_sh);
#endif
}

template <typename T>
int launch(const ParamsI8Var& pv, int block_rows, hipStream_t st) {
  return launch_varlen(attn_i8_varlen_kernel<T, 8>, attn_i8_varlen_kernel<T, 4>, pv.pi.p, pv, block_rows, st);
}

}  // namespace

extern "C" int vorta_attn_fwd_varlen_i8(const vorta_attn_args* a, const vorta_attn_i8_ext* i8, const vorta_attn_varlen_ext* ext,
                                        void* hip_stream) {
  // the ext's size, the int8 entry point's checks (fill_i8), then the variable-length entry point's: each with the return
  // code its parent gives
  if (!varlen_ext_sized(ext)) return VORTA_EINVAL;
  ParamsI8Var pv{};
  int block_rows = 0;
  int rc = fill_i8(a, i8, pv.pi, block_rows);
  if (rc == VORTA_OK) rc = fill_var_tables(a, ext, pv.pi.p, pv.t);
  if (rc != VORTA_OK) return rc;
  if (pv.pi.p.n_heads == 0 || pv.pi.p.n_groups == 0) return VORTA_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  return a->dtype == VORTA_BF16 ? launch<__bf16>(pv, block_rows, st) : launch<_Float16>(pv, block_rows, st);
}
