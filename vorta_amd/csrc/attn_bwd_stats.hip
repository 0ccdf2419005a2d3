// Softmax statistics for the key-major attention backward (include/vorta_hip.h vorta_attn_bwd_stats), gfx950 (MI355X, CDNA4).
// The forward keeps neither the row maximum nor the row sum, and the key-major pass (csrc/attn_bwd_kmajor.hip) needs both,
// plus delta, for every query row before it starts: this is pass 1 of csrc/attn_bwd.hip as a kernel of its own, with the key on
// the MFMA lane as in the key-major pass (csrc/attn_bwd_kmajor.h says why the two must agree).
//
// Query-major, no atomics: a workgroup (4 waves) owns 128 query positions of one (head slot, group) -- the decomposition of
// vorta_attn_bwd -- and walks the group's key list once in 64-key blocks.  A wave forms, for its 32 queries,
//     S = Q . K^T and dP = dO_eff . V^T        (accumulator: 16 queries in a lane's registers, ONE key per lane and half),
// and every lane runs the online softmax of ITS key stripe (keys lane, lane + 32, lane + 64, ... of the list) for its 16
// queries: running maximum m, l = sum exp2(c (s - m)), d = sum exp2(c (s - m)) dP.  The 32 stripes of a query are merged once,
// at the end, with lane shuffles, and the wave writes
//     lse2[p] = m c + log2(l)      delta[p] = d / l = sum_j P[p][j] dP[p][j]
// to stats[head slot][p][0..1].  Positions at or past q_valid_eff have dO_eff = 0, hence delta = 0, and their true lse2.
// LDS: Q 32 K + dO_eff 32 K + K 16 K + V 16 K = 96 KiB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_bwd_kmajor.h"

namespace {
using namespace vorta_attn_km;

constexpr int Q_OFF = 0;
constexpr int DO_OFF = Q_OFF + SQB * ROWB;
constexpr int K_OFF = DO_OFF + SQB * ROWB;
constexpr int V_OFF = K_OFF + TILE_BYTES;
constexpr int STATS_LDS = V_OFF + TILE_BYTES;

__device__ __forceinline__ float half_wave_max(float x) {
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) x = fmaxf(x, __shfl_xor(x, off));
  return x;
}
__device__ __forceinline__ float half_wave_sum(float x) {
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) x += __shfl_xor(x, off);
  return x;
}

template <typename T>
__global__ __launch_bounds__(KNT) void attn_bwd_stats_kernel(const KmParams kp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  using V8 = typename MF<T>::v8;
  constexpr int CH = (KVB * 16) / KNT;  // 16-byte chunks of one K / V tile per thread (4)
  constexpr int ROWSTEP = KNT / 16;     // rows between a thread's consecutive chunks (16)
  const Params& p = kp.p;

  __shared__ __attribute__((aligned(16))) char smem[STATS_LDS];

  // ---- work decomposition (vorta_attn_bwd's) ----
  const int wg = live_order(p, blockIdx.x, gridDim.x, p.xcd_remap);
  const int n_qb = p.n_groups * p.blocks_per_group;
  const int qb = wg % n_qb;
  const int y = wg / n_qb;
  if (p.n_heads_dev && y >= *p.n_heads_dev) return;
  const int head = p.head_list ? p.head_list[y] : y;
  int grp, p0, pend;
  if (p.q_block_table) {
    const int32_t* t = p.q_block_table + 3 * (qb / kp.sub);
    grp = t[0]; p0 = t[1] + (qb % kp.sub) * SQB; pend = t[2];
  } else {
    q_block_of(p, qb, SQB, grp, p0, pend);
  }
  if (p0 >= pend) return;  // (workgroup-uniform)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31;
  const int hh = lane >> 5;

  const int n_kv = p.n_kv_dev ? max(1, min(*p.n_kv_dev, p.n_kv)) : p.n_kv;
  const int q_valid = p.q_valid_dev ? min(*p.q_valid_dev, p.q_valid) : p.q_valid;
  const int nblk = (n_kv + KVB - 1) / KVB;
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)y * p.q_rows_sh : nullptr;
  const int lrow0 = tid >> 4;
  const int lcc = tid & 15;

  // ---- prologue: LDS images of Q and dO_eff ----
  {
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
      *(u32x4*)(smem + Q_OFF + dst) = *(const u32x4*)(qh + r * p.q_ss);
      const V8 g0 = *(const V8*)(gh + r * kp.do_ss);
      *(V8*)(smem + DO_OFF + dst) = do_eff_chunk<T>(kp, g0, gh, y, pos, w, ok);
    }
  }
  __syncthreads();

  // ---- this lane's query row as the A operand: fragments of q and dO_eff ----
  const int my_q = wave * 32 + r32;
  V8 qf[8], gf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    qf[ks] = *(const V8*)(smem + Q_OFF + tile_off(my_q, (2 * ks + hh) * 8));
    gf[ks] = *(const V8*)(smem + DO_OFF + tile_off(my_q, (2 * ks + hh) * 8));
  }

  // ---- K / V loader (global -> registers one block ahead -> LDS) ----
  const int32_t* kv_rows =
      p.kv_rows ? p.kv_rows + (int64_t)y * p.kv_rows_sh + (int64_t)grp * p.kv_rows_sg : nullptr;
  const char* kbase = p.k + (int64_t)head * p.k_sh + lcc * 16;
  const char* vbase = p.v + (int64_t)head * p.v_sh + lcc * 16;
  int t_wr[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) t_wr[i] = tile_off(lrow0 + i * ROWSTEP, lcc * 8);
  u32x4 kreg[CH], vreg[CH];
  int64_t nrow[CH];
#define FETCH_ROWS(blk_)                                                          \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) {                             \
    const int pos_ = min((blk_) * KVB + lrow0 + i_ * ROWSTEP, n_kv - 1);          \
    nrow[i_] = kv_rows ? (int64_t)kv_rows[pos_] : (int64_t)(p.kv_row_offset + pos_); \
  }
#define ISSUE_KV()                                                                \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) {                             \
    kreg[i_] = *(const u32x4*)(kbase + nrow[i_] * p.k_ss);                        \
    vreg[i_] = *(const u32x4*)(vbase + nrow[i_] * p.v_ss);                        \
  }
#define WRITE_KV()                                                                \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) {                             \
    *(u32x4*)(smem + K_OFF + t_wr[i_]) = kreg[i_];                                \
    *(u32x4*)(smem + V_OFF + t_wr[i_]) = vreg[i_];                                \
  }

  // a key's fragments as the B operand: key row r32 (+32), 8 channels (row + 32 keeps row & 15: same offset + 32 rows)
  int k_rd[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) k_rd[ks] = tile_off(r32, (2 * ks + hh) * 8);
#define SCORES(d0_, d1_, off_, a_)                                                \
  {                                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) { d0_[i_] = 0.f; d1_[i_] = 0.f; } \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 8; ++ks_) {                         \
      const V8 b0_ = *(const V8*)(smem + (off_) + k_rd[ks_]);                     \
      const V8 b1_ = *(const V8*)(smem + (off_) + k_rd[ks_] + 32 * ROWB);         \
      d0_ = MF<T>::mfma(a_[ks_], b0_, d0_);                                       \
      d1_ = MF<T>::mfma(a_[ks_], b1_, d1_);                                       \
    }                                                                             \
  }

  const float c = p.scale_log2;

  // ---- the key sweep: register i of an accumulator = query (i & 3) + 8 (i >> 2) + 4 hh of the wave, this lane's key ----
  float m_run[16], l_run[16], d_run[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { m_run[i] = -1e30f; l_run[i] = 0.f; d_run[i] = 0.f; }
  FETCH_ROWS(0);
  ISSUE_KV();
  for (int blk = 0; blk < nblk; ++blk) {
    WRITE_KV();
    __syncthreads();
    if (blk + 1 < nblk) {
      FETCH_ROWS(blk + 1);
      ISSUE_KV();
    }
    f32x16 s0, s1, g0, g1;
    SCORES(s0, s1, K_OFF, qf)
    SCORES(g0, g1, V_OFF, gf)
    const bool dead0 = blk * KVB + r32 >= n_kv, dead1 = blk * KVB + 32 + r32 >= n_kv;  // (the tail of the last block)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float a0 = dead0 ? -INFINITY : s0[i], a1 = dead1 ? -INFINITY : s1[i];
      const float m_new = fmaxf(m_run[i], fmaxf(a0, a1));
      const float alpha = __builtin_amdgcn_exp2f((m_run[i] - m_new) * c);  // exp2(0) = 1 when the maximum stays
      const float mc = rounded_mul(m_new, c);
      const float e0 = expo(a0, c, mc), e1 = expo(a1, c, mc);
      l_run[i] = l_run[i] * alpha + (e0 + e1);
      d_run[i] = d_run[i] * alpha + (e0 * g0[i] + e1 * g1[i]);
      m_run[i] = m_new;
    }
    __syncthreads();
  }
#undef FETCH_ROWS
#undef ISSUE_KV
#undef WRITE_KV
#undef SCORES

  // ---- merge the 32 key stripes of every query (the lanes of one half), write (lse2, delta) ----
  float* st = kp.stats + (int64_t)y * kp.stats_sh;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float m_all = half_wave_max(m_run[i]);
    const float wgt = __builtin_amdgcn_exp2f((m_run[i] - m_all) * c);  // 1 for the stripe(s) that hold the maximum, 0 for an empty one
    const float l_tot = half_wave_sum(l_run[i] * wgt);
    const float d_tot = half_wave_sum(d_run[i] * wgt);
    const bool some = l_tot > 0.f;
    const float lse2 = rounded_mul(m_all, c) + (some ? __builtin_amdgcn_logf(l_tot) : 0.f);
    const float delta = d_tot * (some ? 1.f / l_tot : 0.f);
    const int pos = p0 + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
    if (r32 == i && pos < pend) *(float2*)(st + 2 * (int64_t)pos) = make_float2(lse2, delta);
  }
#endif
}

}  // namespace

extern "C" int vorta_attn_bwd_stats(const vorta_attn_bwd_kmajor_args* a, void* hip_stream) {
  KmParams kp{};
  const int rc = fill_km(a, kp, false);
  if (rc != VORTA_OK) return rc;
  const Params& p = kp.p;
  if (p.n_heads == 0) return VORTA_OK;
  const int64_t total = (int64_t)p.wg_per_slot * p.n_heads;
  if (total > 0x7fffffff) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  if (a->bwd.fwd.dtype == VORTA_BF16) hipLaunchKernelGGL(attn_bwd_stats_kernel<__bf16>, dim3((unsigned)total), dim3(KNT), 0, st, kp);
  else hipLaunchKernelGGL(attn_bwd_stats_kernel<_Float16>, dim3((unsigned)total), dim3(KNT), 0, st, kp);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
