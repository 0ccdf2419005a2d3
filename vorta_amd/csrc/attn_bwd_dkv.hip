// The dK / dV pass of the DETERMINISTIC attention backward for gfx950 (MI355X, CDNA4): include/vorta_hip.h vorta_attn_bwd_dkv.
// The key-major sweep of csrc/attn_bwd_kmajor.hip reduced to what dK and dV need: no dS image, no dQ product, no atomic.  It
// needs the softmax statistics of every query row (vorta_attn_bwd_stats, csrc/attn_bwd_stats.hip); vorta_attn_bwd_dq
// (csrc/attn_bwd_dq.hip) gives dq.
//
// One LAUNCH = one key list (group); one workgroup (4 waves) = one 256-key block of that list for one head slot; wave w keeps
// keys 64 w .. 64 w + 63.  It sweeps the query positions of the group in 32-row slices (with a q_block_table: every table row
// of the group, found by scanning the table).  Per slice, with the key on the MFMA lane (csrc/attn_bwd_kmajor.h: the
// statistics pass forms the same numbers the same way):
//     S = Q . K^T, dP = dO_eff . V^T      (accumulator: 16 queries in a lane's registers, one key per lane and half)
//     P = exp2(c s - lse2)                dS = P (dP - delta)
//     dV[key][d] += P^T . dO_eff          dK[key][d] += dS^T . Q      (the accumulators ARE the A operands; Q and dO_eff come
//                                                                      out of their LDS images through transposed reads)
// At the end of the sweep the workgroup adds scale dK and dV to the fp32 dk / dv rows of its keys with a plain read-add-write.
// The first n_kv_eff rows of one key list are distinct and head_list names distinct heads (include/vorta_hip.h), so inside a
// launch every (head, key row) has ONE writer; key lists of different groups overlap (sliding tile) and the three experts of
// the mixture share the buffers, and those meet in stream order: the host entry point issues the lists' launches one after
// the other on the caller's stream.
// K stays in LDS for the whole sweep (64 KiB), V in registers (it is only ever the B operand of dP).  The Q / dO_eff /
// statistics images of a slice are double-buffered: the next slice is loaded one slice ahead and written into the other
// buffer after this slice's products, so ONE barrier per slice serves the sweep.
//
// REPRODUCIBILITY: dk and dv are bit-reproducible -- no atomic, one writer per row and launch, stream order across launches.
// There is no protocol between workgroups of any kind: a workgroup never depends on another one's progress.
// LDS: K 64 K + 2 x (Q 8 K + dO_eff 8 K + statistics 256) = 96.5 KiB: one workgroup per CU (as the 512 registers per lane
// already make it).
// Registers: as csrc/attn_bwd_kmajor.hip -- dK and dV fill the 256 accumulator registers, and vorta_amd/build.py compiles this
// file with -mllvm -amdgpu-mfma-vgpr-form as well, so that the S / dP results may live in the ordinary registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_bwd_kmajor.h"

namespace {
using namespace vorta_attn_km;

// one slice buffer; two of them first, then the K image (every read is one lane-constant base register, the buffer's
// offset and an immediate)
constexpr int Q_OFF = 0;
constexpr int DO_OFF = Q_OFF + QSL * ROWB;
constexpr int ST_OFF = DO_OFF + QSL * ROWB;  // [32] (lse2, delta)
constexpr int SLB = ST_OFF + QSL * 8;        // bytes of a slice buffer (a multiple of 256: the same banks in both)
constexpr int K_OFF = 2 * SLB;
constexpr int DKV_LDS = K_OFF + KMB * ROWB;

// The next 32-row slice of group grp below q_valid; r = -1 before the first call (r: the table row, or 0).  Table rows of one
// group need not be contiguous or ordered.  Workgroup-uniform.  (csrc/attn_bwd_kmajor.hip sweeps in the same order)
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

template <typename T>
__global__ __launch_bounds__(KNT) void attn_bwd_dkv_kernel(const KmParams kp, const int grp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
  const Params& p = kp.p;

  __shared__ __attribute__((aligned(16))) char smem[DKV_LDS];

  // ---- work decomposition: (head slot, key block) of the launch's key list ----
  const int wg = live_order(p, blockIdx.x, gridDim.x, p.xcd_remap);
  const int kb = wg % kp.n_kblocks;
  const int y = wg / kp.n_kblocks;
  if (p.n_heads_dev && y >= *p.n_heads_dev) return;
  const int head = p.head_list ? p.head_list[y] : y;
  const int n_kv = p.n_kv_dev ? max(1, min(*p.n_kv_dev, p.n_kv)) : p.n_kv;
  const int q_valid = p.q_valid_dev ? min(*p.q_valid_dev, p.q_valid) : p.q_valid;
  if (kb * KMB >= n_kv) return;  // (workgroup-uniform)
  int sl_r = -1, sl_p0 = 0, sl_end = 0;
  if (!next_slice(kp, grp, q_valid, sl_r, sl_p0, sl_end)) return;  // the group has no query below q_valid

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31;
  const int hh = lane >> 5;
  const int lrow0 = tid >> 4;
  const int lcc = tid & 15;
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)y * p.q_rows_sh : nullptr;
  const int32_t* kv_rows =
      p.kv_rows ? p.kv_rows + (int64_t)y * p.kv_rows_sh + (int64_t)grp * p.kv_rows_sg : nullptr;
  const float c = p.scale_log2;
  float w = 1.f;
  if (kp.do_scale) w = (float)((const T*)kp.do_scale)[(int64_t)head * kp.do_scale_sh];

  // ---- the K image of this key block (rows past n_kv repeat the last key: finite, and masked below) ----
  {
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
      for (int i = 0; i < 4; ++i) *(u32x4*)(smem + K_OFF + tile_off(64 * b + lrow0 + 16 * i, lcc * 8)) = kreg[i];
    }
  }
  // ---- this lane's two keys: fragments of v (B operand of dP) ----
  const int key0 = wave * 64 + r32;  // row of the K image; the second key is 32 rows on
  V8 vf[2][8];
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    const int pos = min(kb * KMB + key0 + 32 * kh, n_kv - 1);
    const int64_t row = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
    const char* vr = p.v + (int64_t)head * p.v_sh + row * p.v_ss;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) vf[kh][ks] = *(const V8*)(vr + (2 * ks + hh) * 16);
  }

  // ---- slice loader: global -> registers one slice ahead -> the other LDS buffer ----
  const char* qh = p.q + (int64_t)head * p.q_sh + lcc * 16;
  const char* gh = kp.d_o + (int64_t)head * kp.do_sh + lcc * 16;
  const float* st = kp.stats + (int64_t)y * kp.stats_sh;
  u32x4 qreg[2];
  V8 greg[2];
  float2 sreg;
#define ISSUE_SLICE(p0_, end_)                                                                   \
  {                                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                           \
      const int ldp_ = min((p0_) + lrow0 + 16 * i_, (end_) - 1);                                 \
      const int64_t r_ = q_rows ? (int64_t)q_rows[ldp_] : (int64_t)(p.q_row_offset + ldp_);      \
      qreg[i_] = *(const u32x4*)(qh + r_ * p.q_ss);                                              \
      greg[i_] = *(const V8*)(gh + r_ * kp.do_ss);                                               \
    }                                                                                            \
    if (tid < QSL) {                                                                             \
      const int pos_ = (p0_) + tid;                                                              \
      sreg = make_float2(1e30f, 0.f); /* a position outside the slice: P = exp2(.. - 1e30) = 0 */ \
      if (pos_ < (end_)) sreg = *(const float2*)(st + 2 * (int64_t)pos_);                        \
    }                                                                                            \
  }
#define WRITE_SLICE(p0_, end_, buf_)                                                             \
  {                                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                           \
      const int row_ = lrow0 + 16 * i_;                                                          \
      const int pos_ = (p0_) + row_;                                                             \
      const int dst_ = (buf_) + tile_off(row_, lcc * 8);                                         \
      *(u32x4*)(smem + Q_OFF + dst_) = qreg[i_];                                                 \
      *(V8*)(smem + DO_OFF + dst_) = do_eff_chunk<T>(kp, greg[i_], gh, y, pos_, w, pos_ < (end_)); \
    }                                                                                            \
    if (tid < QSL) *(float2*)(smem + ST_OFF + (buf_) + tid * 8) = sreg;                          \
  }

  // transposed reads (ds_read_b64_tr_b16): a lane addresses row k0 + 4 hh + (lane & 15) / 4, elements n0 + 16 (lane / 16 & 1)
  // + 4 (lane & 3) of a row-major [k][n] image and receives, for n = n0 + r32, the four k = k0 + 4 hh + 0..3; two reads
  // (k0, k0 + 8) fill the eight k slots of a lane -- the order of an accumulator's registers (8 b + j: query 16 b + 4 hh +
  // (j & 3) + 8 (j >> 2)), so an accumulator and such a pair of reads are the two operands of one product
  const int tr_row = 4 * hh + ((lane & 15) >> 2);
  const int tr_col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  // lane-constant LDS bases (tile_off(row + 16 n, e) = tile_off(row, e) + 16 n ROWB)
  int rd[8], krd[8], trd[2][4];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    rd[ks] = tile_off(r32, (2 * ks + hh) * 8);   // a query's (Q / dO_eff image) fragment ks
    krd[ks] = K_OFF + wave * 64 * ROWB + rd[ks]; // this lane's first key (row key0: the same row & 15); the second is 32 rows on
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) trd[h][dt] = tile_off(tr_row + 8 * h, 32 * dt + tr_col);
  const int strd = ST_OFF + 4 * hh * 8;

  f32x16 dk[2][4], dv[2][4];  // [key half][32 channels]: rows = the half's keys, this lane's column = channel 32 dt + r32
#pragma unroll
  for (int kh = 0; kh < 2; ++kh)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dk[kh][dt][i] = 0.f; dv[kh][dt][i] = 0.f; }

  ISSUE_SLICE(sl_p0, sl_end)
  WRITE_SLICE(sl_p0, sl_end, 0)

  bool have = true;
  for (int it = 0; have; ++it) {
    // this slice's images are in place (first turn: the K image too), and every wave is done with the other buffer, which it
    // read a turn ago
    __syncthreads();
    const int cur = (it & 1) * SLB;
    const char* sb = smem + cur;
    int nx_r = sl_r, nx_p0 = sl_p0, nx_end = sl_end;
    const bool have_next = next_slice(kp, grp, q_valid, nx_r, nx_p0, nx_end);
    if (have_next) ISSUE_SLICE(nx_p0, nx_end)

#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      // S and dP of 32 queries x this wave's 32 keys of the half
      f32x16 s, g;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; g[i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const V8 aq = *(const V8*)(sb + rd[ks] + Q_OFF);
        const V8 ag = *(const V8*)(sb + rd[ks] + DO_OFF);
        const V8 bk = *(const V8*)(smem + krd[ks] + 32 * kh * ROWB);
        s = MF<T>::mfma(aq, bk, s);
        g = MF<T>::mfma(ag, vf[kh][ks], g);
      }
      const bool dead = kb * KMB + key0 + 32 * kh >= n_kv;  // (the tail of the last key block)
      V8 pb[2], dsb[2];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float2 sd = *(const float2*)(sb + strd + ((i & 3) + 8 * (i >> 2)) * 8);
        const float pv = dead ? 0.f : expo(s[i], c, sd.x);
        pb[i >> 3][i & 7] = (T)pv;
        dsb[i >> 3][i & 7] = (T)(pv * (g[i] - sd.y));
      }
      // dV[key][d] += P^T . dO_eff, dK[key][d] += dS^T . Q
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int oa = trd[0][dt] + 16 * b * ROWB, oc = trd[1][dt] + 16 * b * ROWB;
          const V4 lo = MF<T>::tr(sb + DO_OFF + oa), hi = MF<T>::tr(sb + DO_OFF + oc);
          const V4 lo2 = MF<T>::tr(sb + Q_OFF + oa), hi2 = MF<T>::tr(sb + Q_OFF + oc);
          V8 xg, xq;
#pragma unroll
          for (int j = 0; j < 4; ++j) { xg[j] = lo[j]; xg[4 + j] = hi[j]; xq[j] = lo2[j]; xq[4 + j] = hi2[j]; }
          dv[kh][dt] = MF<T>::mfma(pb[b], xg, dv[kh][dt]);
          dk[kh][dt] = MF<T>::mfma(dsb[b], xq, dk[kh][dt]);
        }
      }
    }
    if (have_next) WRITE_SLICE(nx_p0, nx_end, SLB - cur)
    have = have_next;
    sl_r = nx_r; sl_p0 = nx_p0; sl_end = nx_end;
  }
#undef ISSUE_SLICE
#undef WRITE_SLICE

  // ---- epilogue: dk[row(key)] += scale dK, dv[row(key)] += dV (this workgroup is the rows' only writer in the launch) ----
  float* dvh = kp.dv + (int64_t)head * kp.dv_sh + r32;
  float* dkh = kp.dk + (int64_t)head * kp.dk_sh + r32;
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pos = kb * KMB + wave * 64 + 32 * kh + (i & 3) + 8 * (i >> 2) + 4 * hh;
      if (pos < n_kv) {
        const int64_t row = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
        float* dvr = dvh + row * kp.dv_ss;
        float* dkr = dkh + row * kp.dk_ss;
        float ov[4], ok[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { ov[dt] = dvr[32 * dt]; ok[dt] = dkr[32 * dt]; }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dvr[32 * dt] = ov[dt] + dv[kh][dt][i];
          dkr[32 * dt] = ok[dt] + dk[kh][dt][i] * kp.scale;
        }
      }
    }
  }
#endif
}

}  // namespace

extern "C" int vorta_attn_bwd_dkv(const vorta_attn_bwd_kmajor_args* a, void* hip_stream) {
  KmParams kp{};
  const int rc = fill_km(a, kp, false);
  if (rc != VORTA_OK) return rc;
  if (!f32_rows_ok(a->bwd.dk) || !f32_rows_ok(a->bwd.dv)) return VORTA_EINVAL;  // (dq is not looked at)
  Params& p = kp.p;
  if (p.n_heads == 0) return VORTA_OK;
  p.wg_per_slot = kp.n_kblocks;  // this kernel's workgroups per head slot (live_order)
  const int64_t total = (int64_t)p.wg_per_slot * p.n_heads;
  if (total > 0x7fffffff) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  // one launch per key list, in list order: rows that two lists share are added to list by list
  for (int grp = 0; grp < kp.n_lists; ++grp) {
    if (a->bwd.fwd.dtype == VORTA_BF16) hipLaunchKernelGGL(attn_bwd_dkv_kernel<__bf16>, dim3((unsigned)total), dim3(KNT), 0, st, kp, grp);
    else hipLaunchKernelGGL(attn_bwd_dkv_kernel<_Float16>, dim3((unsigned)total), dim3(KNT), 0, st, kp, grp);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vorta_set_hip_error(e);
  }
  return VORTA_OK;
}
