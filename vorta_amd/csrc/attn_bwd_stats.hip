// Softmax statistics for the key-major attention backward (include/vorta_hip.h vorta_attn_bwd_stats), gfx950 (MI355X, CDNA4).
// The forward keeps neither the row maximum nor the row sum, and the key-major pass (csrc/attn_bwd_kmajor.hip) needs both,
// plus delta, for every query row before it starts: this is pass 1 of csrc/attn_bwd.hip as a kernel of its own, with the key on
// the MFMA lane as in the key-major pass (csrc/attn_bwd_kmajor.h says why the two must agree).
//
// Query-major, no atomics: a workgroup (4 waves) owns 128 query positions of one (head slot, group) -- the decomposition of
// vorta_attn_bwd -- and walks the group's key list once in 64-key blocks.  The frame -- decomposition, Q / dO_eff prologue,
// K / V loader, scores() -- is the QUERY-BLOCK PIECES section of csrc/attn_bwd_kmajor.h, shared with csrc/attn_bwd_dq.hip.  A
// wave forms, for its 32 queries,
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
  const Params& p = kp.p;

  __shared__ __attribute__((aligned(16))) char smem[STATS_LDS];

  int y, head, grp, p0, pend;
  if (!q_block_work(kp, y, head, grp, p0, pend)) return;
  if (p0 >= pend) return;  // (workgroup-uniform)

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r32 = lane & 31;
  const int hh = lane >> 5;

  const int n_kv = p.n_kv_dev ? max(1, min(*p.n_kv_dev, p.n_kv)) : p.n_kv;
  const int q_valid = p.q_valid_dev ? min(*p.q_valid_dev, p.q_valid) : p.q_valid;
  const int nblk = (n_kv + KVB - 1) / KVB;
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)y * p.q_rows_sh : nullptr;

  load_q_images<T>(kp, smem, Q_OFF, DO_OFF, y, head, q_rows, p0, pend, q_valid);
  __syncthreads();
  V8 qf[8], gf[8];
  q_frags<T>(smem, Q_OFF, DO_OFF, wave, qf, gf);

  const int32_t* kv_rows =
      p.kv_rows ? p.kv_rows + (int64_t)y * p.kv_rows_sh + (int64_t)grp * p.kv_rows_sg : nullptr;
  KvLoader kv(p, kv_rows, head, n_kv);
  int k_rd[8];
  frag_bases(k_rd);

  const float c = p.scale_log2;

  // ---- the key sweep: register i of an accumulator = query acc_row(i, hh) of the wave, this lane's key ----
  float m_run[16], l_run[16], d_run[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { m_run[i] = -1e30f; l_run[i] = 0.f; d_run[i] = 0.f; }
  kv.rows(0);
  kv.issue();
  for (int blk = 0; blk < nblk; ++blk) {
    kv.write(smem, K_OFF, V_OFF);
    __syncthreads();
    if (blk + 1 < nblk) {
      kv.rows(blk + 1);
      kv.issue();
    }
    f32x16 s0, s1, g0, g1;
    scores<T>(smem, K_OFF, k_rd, qf, s0, s1);
    scores<T>(smem, V_OFF, k_rd, gf, g0, g1);
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
    const int pos = p0 + wave * 32 + acc_row(i, hh);
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
  return launch_km(a, attn_bwd_stats_kernel<__bf16>, attn_bwd_stats_kernel<_Float16>, (int64_t)p.wg_per_slot * p.n_heads,
                   hip_stream, kp);
}
