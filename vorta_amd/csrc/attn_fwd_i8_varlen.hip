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
//     NULL: the family's XCD-aware index order.
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
  const int32_t* kv_len; int64_t kv_len_sh;  // [slot][group]
  const int32_t* order;                      // [grid] or null
};

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_i8_varlen_kernel(const ParamsI8Var pv) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  __shared__ __attribute__((aligned(16))) char smem[SMEM_I8];
  int wg;
  if (pv.order) {
    // (clamped into the grid: an entry that is no workgroup id computes some workgroup twice, it reaches no other memory)
    wg = min(max(__builtin_amdgcn_readfirstlane(pv.order[blockIdx.x]), 0), (int)gridDim.x - 1);
  } else {
    wg = live_order(pv.pi.p, blockIdx.x, gridDim.x, pv.pi.p.xcd_remap);
  }
  attn_i8_body<T, NW, true, NSI8, true>(pv.pi, smem, wg, pv.kv_len, pv.kv_len_sh);
#endif
}

// the int8 entry point's checks (fill_i8), then the variable-length entry point's (attn_fwd_varlen.hip fill_varlen), each
// with the return code its parent gives
int fill_i8_varlen(const vorta_attn_args* a, const vorta_attn_i8_ext* i8, const vorta_attn_varlen_ext* ext, ParamsI8Var& pv,
                   int& block_rows) {
  if (!ext || ext->struct_size != sizeof(vorta_attn_varlen_ext)) return VORTA_EINVAL;
  const int rc = fill_i8(a, i8, pv.pi, block_rows);
  if (rc != VORTA_OK) return rc;
  const Params& p = pv.pi.p;
  if (p.n_heads == 0 || p.n_groups == 0) return VORTA_OK;
  // no split keys (the lengths differ per group, a split of n_kv does not divide them) and no duplicate rows
  if (a->variant == 1 || a->n_splits != 1 || a->dup_rows) return VORTA_EUNSUPPORTED;
  if (!a->kv_rows || !ext->kv_len || ((uintptr_t)ext->kv_len & 3) || ((uintptr_t)ext->order & 3)) return VORTA_EINVAL;
  // (with a q_block_table the number of key lists is the caller's: the stride is checked against q_group_len's groups only)
  if (ext->kv_len_stride_h < (a->q_block_table ? 1 : p.n_groups)) return VORTA_EINVAL;
  pv.kv_len = ext->kv_len; pv.kv_len_sh = ext->kv_len_stride_h; pv.order = ext->order;
  return VORTA_OK;
}

template <typename T>
int launch_i8_varlen(const ParamsI8Var& pv, int block_rows, hipStream_t st) {
  const Params& p = pv.pi.p;
  const int64_t total = (int64_t)p.n_groups * p.blocks_per_group * p.n_heads;
  if (total > 0x7fffffff) return VORTA_EINVAL;
  if (block_rows == 256) hipLaunchKernelGGL((attn_i8_varlen_kernel<T, 8>), dim3((unsigned)total), dim3(512), 0, st, pv);
  else hipLaunchKernelGGL((attn_i8_varlen_kernel<T, 4>), dim3((unsigned)total), dim3(256), 0, st, pv);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

}  // namespace

extern "C" int vorta_attn_fwd_varlen_i8(const vorta_attn_args* a, const vorta_attn_i8_ext* i8, const vorta_attn_varlen_ext* ext,
                                        void* hip_stream) {
  ParamsI8Var pv{};
  int block_rows = 0;
  const int rc = fill_i8_varlen(a, i8, ext, pv, block_rows);
  if (rc != VORTA_OK) return rc;
  if (pv.pi.p.n_heads == 0 || pv.pi.p.n_groups == 0) return VORTA_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  return a->dtype == VORTA_BF16 ? launch_i8_varlen<__bf16>(pv, block_rows, st) : launch_i8_varlen<_Float16>(pv, block_rows, st);
}
