// Shared by the two kernels of the KEY-MAJOR attention backward (include/vorta_hip.h vorta_attn_bwd_stats and
// vorta_attn_bwd_kmajor; csrc/attn_bwd_stats.hip, csrc/attn_bwd_kmajor.hip): the parameter block, the host validation, the LDS
// tile addressing, the exponent and the dO_eff rows.  Both kernels must form the scores and dP from the SAME operands through the
// SAME MFMA chain (A = a query's 8-channel fragments of q / dO_eff, B = a key's fragments of k / v, channel group 2 ks + hh in
// step ks = 0..7, zero initial accumulator): the second kernel takes exp2(c s - lse2) and dP - delta against the first one's
// numbers, and a row with ONE key must come out as P = 1 and dS = 0 exactly, as float64 autograd gives it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"

namespace vorta_attn_km {
using namespace vorta_attn;

constexpr int SQB = 128;  // statistics pass: query rows per workgroup (4 waves of 32)
constexpr int KMB = 256;  // key-major pass: keys per workgroup (4 waves of 64)
constexpr int QSL = 32;   // key-major pass: query rows per slice
constexpr int KNT = 256;  // threads of either kernel

struct KmParams {
  Params p;  // the forward launch, cut into 128-row query blocks (the statistics pass's grid)
  const char* d_o; int64_t do_sh, do_ss;      // bytes
  const void* do_scale; int64_t do_scale_sh;  // elements
  float* dq; float* dk; float* dv;
  int64_t dq_sh, dq_ss, dk_sh, dk_ss, dv_sh, dv_ss;  // floats
  float scale;
  int sub;         // with a q_block_table: 128-row workgroups per table row (statistics pass)
  float* stats; int64_t stats_sh;  // [head slot][position][2] = (lse2, delta); floats per head slot
  int n_lists;     // key lists = query groups
  int n_tab_rows;  // rows of the q_block_table
  int n_kblocks;   // 256-key blocks of the host n_kv
};

// byte offset of 16-bit element (row, ecol) of a 256-byte-row tile: 16-byte chunks XOR-swizzled with the row
__device__ __forceinline__ int tile_off(int row, int ecol) {
  const int bc = ecol * 2;
  return row * ROWB + (((bc >> 4) ^ (row & 15)) << 4) + (bc & 15);
}

// exp2(s c - mc) with the product rounded BEFORE the subtraction (no fused multiply-add): both kernels get the same bits
// from the same score, and a row's only key gives exp2(0) = 1 exactly
__device__ __forceinline__ float rounded_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float expo(float s, float c, float mc) {
#pragma clang fp contract(off)
  const float t = s * c;
  return __builtin_amdgcn_exp2f(t - mc);
}

// 8 channels of dO_eff[pos] = w (d_o[r] + sum_i d_o[dup_rows[y][pos][i]]), rounded to 16 bits; gh = d_o + head offset + the
// chunk's byte offset.  Zero when !ok (positions at or past q_valid_eff, or outside the group).
// (g0 = the 8 channels of d_o[r], loaded by the caller -- ahead of time in the key-major sweep)
template <typename T>
__device__ __forceinline__ typename MF<T>::v8 do_eff_chunk(const KmParams& kp, typename MF<T>::v8 g0, const char* gh, int y,
                                                           int pos, float w, bool ok) {
  using V8 = typename MF<T>::v8;
  const Params& p = kp.p;
  V8 g8;
  if (ok) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (float)g0[e];
    if (p.dup_rows && pos < p.n_dup_pos) {
      const int32_t* dr = p.dup_rows + (int64_t)y * p.dup_rows_sh + (int64_t)pos * p.n_dup;
      for (int j = 0; j < p.n_dup; ++j) {
        const V8 gj = *(const V8*)(gh + (int64_t)dr[j] * kp.do_ss);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)gj[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) g8[e] = (T)(acc[e] * w);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) g8[e] = (T)0.f;
  }
  return g8;
}

inline bool f32_rows_ok(const vorta_tensor& t) {
  return t.ptr && !((uintptr_t)t.ptr & 15) && t.stride_s % 4 == 0 && t.stride_h % 4 == 0 && t.stride_s >= D;
}

// Validation and geometry of either entry point.  VORTA_OK with kp.p.n_heads == 0: a valid block with nothing to launch.
inline int fill_km(const vorta_attn_bwd_kmajor_args* a, KmParams& kp, bool need_grads) {
  if (!a || a->struct_size != sizeof(vorta_attn_bwd_kmajor_args)) return VORTA_EINVAL;
  const vorta_attn_bwd_args& b = a->bwd;
  if (b.struct_size != sizeof(vorta_attn_bwd_args)) return VORTA_EINVAL;
  vorta_attn_args f = b.fwd;  // as vorta_attn_bwd: split keys, workspaces and the forward's kernel variant change nothing
  f.n_splits = 1; f.ws_o = nullptr; f.ws_ml = nullptr;
  f.variant = 1;
  int block_rows = 0;
  int rc = fill_params(&f, kp.p, block_rows, 2);
  if (rc != VORTA_OK) return rc;
  Params& p = kp.p;
  if (p.n_heads == 0 || p.n_groups == 0) { p.n_heads = 0; return VORTA_OK; }
  kp.sub = 1;
  if (f.q_block_table) {
    if (a->n_key_lists <= 0) return VORTA_EINVAL;
    kp.n_lists = a->n_key_lists;
    kp.n_tab_rows = f.n_q_blocks;
    kp.sub = block_rows / SQB;
    p.n_groups *= kp.sub;
  } else {
    if (a->n_key_lists < 0) return VORTA_EINVAL;
    if (block_rows != SQB) {
      f.block_rows = SQB;
      rc = fill_params(&f, p, block_rows, 2);
      if (rc != VORTA_OK) return rc;
    }
    kp.n_lists = p.n_groups;
    kp.n_tab_rows = 0;
  }
  p.n_splits = 1;
  p.wg_per_slot = p.n_groups * p.blocks_per_group;
  kp.n_kblocks = (p.n_kv + KMB - 1) / KMB;
  const vorta_tensor& g = b.d_o;
  if (!g.ptr || ((uintptr_t)g.ptr & 15) || (g.stride_s % 8) || (g.stride_h % 8) || g.stride_s < D) return VORTA_EINVAL;
  if (!a->stats || ((uintptr_t)a->stats & 7) || (a->stats_stride_h % 2) || a->stats_stride_h < 2 * (int64_t)p.n_q)
    return VORTA_EINVAL;
  if (need_grads && (!f32_rows_ok(b.dq) || !f32_rows_ok(b.dk) || !f32_rows_ok(b.dv))) return VORTA_EINVAL;
  kp.d_o = (const char*)g.ptr; kp.do_sh = g.stride_h * 2; kp.do_ss = g.stride_s * 2;
  kp.do_scale = b.do_scale; kp.do_scale_sh = b.do_scale_stride_h;
  kp.dq = (float*)b.dq.ptr; kp.dk = (float*)b.dk.ptr; kp.dv = (float*)b.dv.ptr;
  kp.dq_sh = b.dq.stride_h; kp.dq_ss = b.dq.stride_s;
  kp.dk_sh = b.dk.stride_h; kp.dk_ss = b.dk.stride_s;
  kp.dv_sh = b.dv.stride_h; kp.dv_ss = b.dv.stride_s;
  kp.scale = f.scale;
  kp.stats = a->stats; kp.stats_sh = a->stats_stride_h;
  return VORTA_OK;
}

}  // namespace vorta_attn_km
