// Shared by the four attention-backward kernels that work from the softmax statistics (include/vorta_hip.h vorta_attn_bwd_stats,
// vorta_attn_bwd_kmajor, vorta_attn_bwd_dq, vorta_attn_bwd_dkv): the parameter block, the host validation and launch, the LDS
// tile addressing, the exponent, the dO_eff rows, and the blocks two of the kernels run as the same text:
//   QUERY-BLOCK PIECES   csrc/attn_bwd_stats.hip, csrc/attn_bwd_dq.hip: a workgroup owns 128 query positions and walks a key list
//   KEY-BLOCK SWEEP      csrc/attn_bwd_kmajor.hip, csrc/attn_bwd_dkv.hip: a workgroup owns 256 keys and sweeps 32-query slices
// Every kernel keeps its own LDS map, loop, barriers and epilogue; LDS places are passed as integer offsets from the kernel's
// one LDS base, so that an access stays one lane-constant base register plus an immediate.
// All four must form the scores and dP from the SAME operands through the SAME MFMA chain (A = a query's 8-channel fragments of
// q / dO_eff, B = a key's fragments of k / v, channel group 2 ks + hh in step ks = 0..7, zero initial accumulator: scores() and
// sweep_scores() below): the later kernels take exp2(c s - lse2) and dP - delta against the statistics pass's numbers, and a
// row with ONE key must come out as P = 1 and dS = 0 exactly, as float64 autograd gives it.
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
constexpr int ROWSTEP = KNT / 16;  // rows between a thread's consecutive 16-byte chunks of a tile image (16 chunks per row)

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

// exp2(s c - mc) with the product rounded BEFORE the subtraction (no fused multiply-add): all kernels get the same bits
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

// Validation and geometry of every entry point.  VORTA_OK with kp.p.n_heads == 0: a valid block with nothing to launch.
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

// The launch of an entry point: total workgroups of KNT threads of the kernel of the forward's dtype
template <typename... A>
inline int launch_km(const vorta_attn_bwd_kmajor_args* a, void (*bf16)(A...), void (*fp16)(A...), int64_t total, void* hip_stream,
                     A... args) {
  if (total > 0x7fffffff) return VORTA_EINVAL;
  hipLaunchKernelGGL(a->bwd.fwd.dtype == VORTA_BF16 ? bf16 : fp16, dim3((unsigned)total), dim3(KNT), 0, (hipStream_t)hip_stream,
                     args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

// Register i of a 32 x 32 accumulator = row acc_row(i, hh) of the MFMA's A operand (hh = lane / 32), column lane & 31
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// Fragment ks (channels 8 (2 ks + hh) ..) of row lane & 31 of a tile image, as an MFMA operand; row + 16 n keeps row & 15, so
// the rows 16 n further on are the same offsets + 16 n ROWB
__device__ __forceinline__ void frag_bases(int (&rd)[8]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) rd[ks] = tile_off(lane & 31, (2 * ks + (lane >> 5)) * 8);
}

// Transposed reads (ds_read_b64_tr_b16): a lane addresses row k0 + tr_row(), elements n0 + tr_col() .. + 3 of a row-major
// [k][n] image and receives, for n = n0 + (lane & 31), the four k = k0 + 4 hh + 0..3; two reads (k0, k0 + 8) fill the eight k
// slots of a lane -- the order of an accumulator's registers (8 b + j: row 16 b + acc_row(j, hh)), so an accumulator and such
// a pair of reads are the two operands of one product, and two such pairs have the same k order
__device__ __forceinline__ int tr_row() { return 4 * ((threadIdx.x & 63) >> 5) + ((threadIdx.x & 15) >> 2); }
__device__ __forceinline__ int tr_col() { return 16 * ((threadIdx.x >> 4) & 1) + 4 * (threadIdx.x & 3); }

// ================================ QUERY-BLOCK PIECES (attn_bwd_stats.hip, attn_bwd_dq.hip) ================================

// Work decomposition (vorta_attn_bwd's): the workgroup's head slot y, head, group and query positions p0 .. pend of its 128-row
// block.  False: the head slot is past the device head count.  Workgroup-uniform.
__device__ __forceinline__ bool q_block_work(const KmParams& kp, int& y, int& head, int& grp, int& p0, int& pend) {
  const Params& p = kp.p;
  const int wg = live_order(p, blockIdx.x, gridDim.x, p.xcd_remap);
  const int n_qb = p.n_groups * p.blocks_per_group;
  const int qb = wg % n_qb;
  y = wg / n_qb;
  if (p.n_heads_dev && y >= *p.n_heads_dev) return false;
  head = p.head_list ? p.head_list[y] : y;
  if (p.q_block_table) {
    const int32_t* t = p.q_block_table + 3 * (qb / kp.sub);
    grp = t[0]; p0 = t[1] + (qb % kp.sub) * SQB; pend = t[2];
  } else {
    q_block_of(p, qb, SQB, grp, p0, pend);
  }
  return true;
}

// Prologue: the LDS images of Q and dO_eff of positions p0 .. p0 + 127 (a barrier later: q_frags)
template <typename T>
__device__ __forceinline__ void load_q_images(const KmParams& kp, char* smem, int q_off, int do_off, int y, int head,
                                              const int32_t* q_rows, int p0, int pend, int q_valid) {
  using V8 = typename MF<T>::v8;
  const Params& p = kp.p;
  const int lrow0 = threadIdx.x >> 4, lcc = threadIdx.x & 15;
  float w = 1.f;
  if (kp.do_scale) w = (float)((const T*)kp.do_scale)[(int64_t)head * kp.do_scale_sh];
  const char* qh = p.q + (int64_t)head * p.q_sh + lcc * 16;
  const char* gh = kp.d_o + (int64_t)head * kp.do_sh + lcc * 16;
  for (int i = 0; i < SQB / ROWSTEP; ++i) {
    const int row = lrow0 + i * ROWSTEP;
    const int pos = p0 + row;
    const bool ok = pos < pend && pos < q_valid;
    const int ldp = min(pos, pend - 1);
    const int64_t r = q_rows ? (int64_t)q_rows[ldp] : (int64_t)(p.q_row_offset + ldp);
    const int dst = tile_off(row, lcc * 8);
    *(u32x4*)(smem + q_off + dst) = *(const u32x4*)(qh + r * p.q_ss);
    const V8 g0 = *(const V8*)(gh + r * kp.do_ss);
    *(V8*)(smem + do_off + dst) = do_eff_chunk<T>(kp, g0, gh, y, pos, w, ok);
  }
}
// This lane's query row (32 wave + lane & 31) as the A operand: fragments of q and dO_eff
template <typename T>
__device__ __forceinline__ void q_frags(const char* smem, int q_off, int do_off, int wave, typename MF<T>::v8 (&qf)[8],
                                        typename MF<T>::v8 (&gf)[8]) {
  using V8 = typename MF<T>::v8;
  const int my_q = wave * 32 + (threadIdx.x & 31), hh = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    qf[ks] = *(const V8*)(smem + q_off + tile_off(my_q, (2 * ks + hh) * 8));
    gf[ks] = *(const V8*)(smem + do_off + tile_off(my_q, (2 * ks + hh) * 8));
  }
}

// K / V loader of 64-key blocks: global -> registers one block ahead -> LDS tiles
struct KvLoader {
  static constexpr int CH = (KVB * 16) / KNT;  // 16-byte chunks of one K / V tile per thread (4)
  const Params& p;
  const int32_t* kv_rows;
  const int n_kv;
  const char* kbase; const char* vbase;
  int t_wr[CH];
  int64_t nrow[CH];
  u32x4 kreg[CH], vreg[CH];
  __device__ __forceinline__ KvLoader(const Params& p_, const int32_t* kv_rows_, int head, int n_kv_)
      : p(p_), kv_rows(kv_rows_), n_kv(n_kv_) {
    const int lcc = threadIdx.x & 15;
    kbase = p.k + (int64_t)head * p.k_sh + lcc * 16;
    vbase = p.v + (int64_t)head * p.v_sh + lcc * 16;
#pragma unroll
    for (int i = 0; i < CH; ++i) t_wr[i] = tile_off((threadIdx.x >> 4) + i * ROWSTEP, lcc * 8);
  }
  __device__ __forceinline__ void rows(int blk) {  // (rows past n_kv repeat the last key: finite, and masked by the caller)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int pos = min(blk * KVB + (int)(threadIdx.x >> 4) + i * ROWSTEP, n_kv - 1);
      nrow[i] = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
    }
  }
  __device__ __forceinline__ void issue() {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      kreg[i] = *(const u32x4*)(kbase + nrow[i] * p.k_ss);
      vreg[i] = *(const u32x4*)(vbase + nrow[i] * p.v_ss);
    }
  }
  __device__ __forceinline__ void write(char* smem, int k_off, int v_off) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      *(u32x4*)(smem + k_off + t_wr[i]) = kreg[i];
      *(u32x4*)(smem + v_off + t_wr[i]) = vreg[i];
    }
  }
};

// d0 / d1 = the products of this lane's query fragments a with key lane & 31 / 32 + (lane & 31) of the tile at off (k_rd:
// frag_bases): S from the K tile and q, dP from the V tile and dO_eff
template <typename T>
__device__ __forceinline__ void scores(const char* smem, int off, const int (&k_rd)[8], const typename MF<T>::v8 (&a)[8],
                                       f32x16& d0, f32x16& d1) {
  using V8 = typename MF<T>::v8;
#pragma unroll
  for (int i = 0; i < 16; ++i) { d0[i] = 0.f; d1[i] = 0.f; }
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const V8 b0 = *(const V8*)(smem + off + k_rd[ks]);
    const V8 b1 = *(const V8*)(smem + off + k_rd[ks] + 32 * ROWB);
    d0 = MF<T>::mfma(a[ks], b0, d0);
    d1 = MF<T>::mfma(a[ks], b1, d1);
  }
}

// ================================ KEY-BLOCK SWEEP (attn_bwd_kmajor.hip, attn_bwd_dkv.hip) ================================
// One workgroup = one 256-key block of a key list, wave w keeps keys 64 w .. 64 w + 63 (a lane: keys 64 w + (lane & 31) and
// 32 on); K stays in LDS for the sweep, V in registers; the group's queries pass in 32-row slices.

// a slice buffer starts with the Q and the dO_eff image; its statistics [32] (lse2, delta) lie where the kernel says
constexpr int SL_Q = 0;
constexpr int SL_DO = SL_Q + QSL * ROWB;

// The next 32-row slice of group grp below q_valid; r = -1 before the first call (r: the table row, or 0).  Table rows of one
// group need not be contiguous or ordered.  Workgroup-uniform.
__device__ __forceinline__ bool next_slice(const KmParams& kp, int grp, int q_valid, int& r, int& p0, int& end) {
  const Params& p = kp.p;
  if (r >= 0) {
    p0 += QSL;
    if (p0 < end) return true;
  }
  if (!p.q_block_table) {
    if (r >= 0) return false;
    r = 0;
    p0 = grp * p.q_group_len;
    end = min(min(p0 + p.q_group_len, p.n_q), q_valid);
    return p0 < end;
  }
  for (++r; r < kp.n_tab_rows; ++r) {
    const int32_t* t = p.q_block_table + 3 * r;
    if (t[0] != grp) continue;
    p0 = t[1];
    end = min(min(t[2], p.n_q), q_valid);
    if (p0 < end) return true;
  }
  return false;
}

// The K image of key block kb at k_off (rows past n_kv repeat the last key: finite, and masked by `dead` below)
__device__ __forceinline__ void load_k_image(const Params& p, char* smem, int k_off, const int32_t* kv_rows, int head, int kb,
                                             int n_kv) {
  const int lrow0 = threadIdx.x >> 4, lcc = threadIdx.x & 15;
  const char* kbase = p.k + (int64_t)head * p.k_sh + lcc * 16;
#pragma unroll 1
  for (int b = 0; b < KMB / 64; ++b) {
    u32x4 kreg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pos = min(kb * KMB + 64 * b + lrow0 + 16 * i, n_kv - 1);
      const int64_t row = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
      kreg[i] = *(const u32x4*)(kbase + row * p.k_ss);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *(u32x4*)(smem + k_off + tile_off(64 * b + lrow0 + 16 * i, lcc * 8)) = kreg[i];
  }
}

// This lane's two keys (positions pos0 and pos0 + 32 of the list): fragments of v, the B operand of dP
template <typename T>
__device__ __forceinline__ void load_v_frags(const Params& p, const int32_t* kv_rows, int head, int pos0, int n_kv,
                                             typename MF<T>::v8 (&vf)[2][8]) {
  using V8 = typename MF<T>::v8;
  const int hh = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    const int pos = min(pos0 + 32 * kh, n_kv - 1);
    const int64_t row = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
    const char* vr = p.v + (int64_t)head * p.v_sh + row * p.v_ss;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) vf[kh][ks] = *(const V8*)(vr + (2 * ks + hh) * 16);
  }
}

// Slice loader: global -> registers one slice ahead -> the slice buffer at buf (q, dO_eff, and the statistics at buf + st_off).
// ROWS (the key-major kernel): the dq row of every position, -1 = none, goes to row_off as well.
template <typename T, bool ROWS>
struct SliceLoader {
  using V8 = typename MF<T>::v8;
  const KmParams& kp;
  const int32_t* q_rows;
  const int y;
  const float w;
  const char* qh; const char* gh;
  const float* st;
  u32x4 qreg[2];
  V8 greg[2];
  float2 sreg;
  int64_t rreg;
  __device__ __forceinline__ SliceLoader(const KmParams& kp_, const int32_t* q_rows_, int y_, int head, float w_)
      : kp(kp_), q_rows(q_rows_), y(y_), w(w_) {
    qh = kp.p.q + (int64_t)head * kp.p.q_sh + (threadIdx.x & 15) * 16;
    gh = kp.d_o + (int64_t)head * kp.do_sh + (threadIdx.x & 15) * 16;
    st = kp.stats + (int64_t)y * kp.stats_sh;
  }
  __device__ __forceinline__ void issue(int p0, int end) {
    const Params& p = kp.p;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ldp = min(p0 + (tid >> 4) + 16 * i, end - 1);
      const int64_t r = q_rows ? (int64_t)q_rows[ldp] : (int64_t)(p.q_row_offset + ldp);
      qreg[i] = *(const u32x4*)(qh + r * p.q_ss);
      greg[i] = *(const V8*)(gh + r * kp.do_ss);
    }
    if (tid < QSL) {
      const int pos = p0 + tid;
      sreg = make_float2(1e30f, 0.f);  // a position outside the slice: P = exp2(.. - 1e30) = 0
      if (ROWS) rreg = -1;
      if (pos < end) {
        sreg = *(const float2*)(st + 2 * (int64_t)pos);
        if (ROWS) rreg = q_rows ? (int64_t)q_rows[pos] : (int64_t)(p.q_row_offset + pos);
      }
    }
  }
  __device__ __forceinline__ void write(char* smem, int p0, int end, int buf, int st_off, int row_off = 0) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (tid >> 4) + 16 * i;
      const int pos = p0 + row;
      const int dst = buf + tile_off(row, (tid & 15) * 8);
      *(u32x4*)(smem + SL_Q + dst) = qreg[i];
      *(V8*)(smem + SL_DO + dst) = do_eff_chunk<T>(kp, greg[i], gh, y, pos, w, pos < end);
    }
    if (tid < QSL) {
      *(float2*)(smem + st_off + buf + tid * 8) = sreg;
      if (ROWS) *(int64_t*)(smem + row_off + tid * 8) = rreg;
    }
  }
};

// Lane-constant LDS bases of the sweep; everything else is an immediate
struct SweepBases {
  int rd[8];      // a query's (Q / dO_eff image) fragment ks: frag_bases
  int krd[8];     // the same fragment of this lane's first key in the K image (row 64 wave + lane & 31: the same row & 15)
  int trd[2][4];  // transposed reads of a slice image: rows tr_row() + 8 h, channels 32 dt ..
  __device__ __forceinline__ SweepBases(int wave, int k_off) {
    frag_bases(rd);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) krd[ks] = k_off + wave * 64 * ROWB + rd[ks];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) trd[h][dt] = tile_off(tr_row() + 8 * h, 32 * dt + tr_col());
  }
};

// S and dP of the slice's 32 queries x this wave's 32 keys of half kh, then P = exp2(c s - lse2) and dS = P (dP - delta) in
// 16 bits: pb / dsb [b] = queries 16 b + acc_row(j, hh) of this lane's key.  sb = the slice buffer, strd = its statistics + 32 hh.
template <typename T>
__device__ __forceinline__ void sweep_scores(const char* smem, const char* sb, const SweepBases& lb, int kh,
                                             const typename MF<T>::v8 (&vf)[8], int strd, bool dead, float c,
                                             typename MF<T>::v8 (&pb)[2], typename MF<T>::v8 (&dsb)[2]) {
  using V8 = typename MF<T>::v8;
  f32x16 s, g;
#pragma unroll
  for (int i = 0; i < 16; ++i) { s[i] = 0.f; g[i] = 0.f; }
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const V8 aq = *(const V8*)(sb + lb.rd[ks] + SL_Q);
    const V8 ag = *(const V8*)(sb + lb.rd[ks] + SL_DO);
    const V8 bk = *(const V8*)(smem + lb.krd[ks] + 32 * kh * ROWB);
    s = MF<T>::mfma(aq, bk, s);
    g = MF<T>::mfma(ag, vf[ks], g);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float2 sd = *(const float2*)(sb + strd + acc_row(i, 0) * 8);
    const float pv = dead ? 0.f : expo(s[i], c, sd.x);
    pb[i >> 3][i & 7] = (T)pv;
    dsb[i >> 3][i & 7] = (T)(pv * (g[i] - sd.y));
  }
}

// dV[key][d] += P^T . dO_eff, dK[key][d] += dS^T . Q: the accumulators' values ARE the A operands, Q and dO_eff come out of
// their images through transposed reads
template <typename T>
__device__ __forceinline__ void sweep_dkv(const char* sb, const SweepBases& lb, const typename MF<T>::v8 (&pb)[2],
                                          const typename MF<T>::v8 (&dsb)[2], f32x16 (&dv)[4], f32x16 (&dk)[4]) {
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int oa = lb.trd[0][dt] + 16 * b * ROWB, oc = lb.trd[1][dt] + 16 * b * ROWB;
      const V4 lo = MF<T>::tr(sb + SL_DO + oa), hi = MF<T>::tr(sb + SL_DO + oc);
      const V4 lo2 = MF<T>::tr(sb + SL_Q + oa), hi2 = MF<T>::tr(sb + SL_Q + oc);
      V8 xg, xq;
#pragma unroll
      for (int j = 0; j < 4; ++j) { xg[j] = lo[j]; xg[4 + j] = hi[j]; xq[j] = lo2[j]; xq[4 + j] = hi2[j]; }
      dv[dt] = MF<T>::mfma(pb[b], xg, dv[dt]);
      dk[dt] = MF<T>::mfma(dsb[b], xq, dk[dt]);
    }
  }
}

}  // namespace vorta_attn_km
