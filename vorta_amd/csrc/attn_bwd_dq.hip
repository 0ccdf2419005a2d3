// The dQ pass of the DETERMINISTIC attention backward for gfx950 (MI355X, CDNA4): include/vorta_hip.h vorta_attn_bwd_dq.  The
// same dq as vorta_attn_bwd (csrc/attn_bwd.hip), from the softmax statistics vorta_attn_bwd_stats wrote (csrc/attn_bwd_stats.hip)
// instead of a first sweep of its own; vorta_attn_bwd_dkv (csrc/attn_bwd_dkv.hip) gives dk and dv.
//
// Query-major, no atomics: a workgroup (4 waves) owns 128 query positions of one (head slot, group) -- the statistics pass's
// grid and decomposition -- and walks the group's key list once in 64-key blocks (the frame is the statistics pass's: the
// QUERY-BLOCK PIECES section of csrc/attn_bwd_kmajor.h).  A wave forms, for its 32 queries and with the key on the MFMA lane,
//     S = Q . K^T, dP = dO_eff . V^T      (accumulator: 16 queries in a lane's registers, one key per lane and half)
//     P = exp2(c s - lse2)                dS = P (dP - delta)
// writes dS, 16 bits, as a [key][query] image of its own (64 keys x 32 queries; no other wave reads it, so no barrier serves
// it) and takes
//     dQ[q][d] += sum over the block's 64 keys of dS[q][key] K[key][d]
// with both operands out of LDS through transposed reads (the dS image and the K tile the scores were formed from).  At the
// end every wave adds scale dQ to the fp32 dq rows of its positions with a plain read-add-write: one workgroup per row, as in
// vorta_attn_bwd.  Positions at or past q_valid_eff, and rows the launch does not name, receive nothing.
//
// REPRODUCIBILITY: dq is bit-reproducible -- no atomic, one writer per row, and a fixed summation order inside the writer.
// LDS: dS 20 K + K 16 K + V 16 K + Q 32 K + dO_eff 32 K = 116 KiB (Q and dO_eff are only read once, into registers).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_bwd_kmajor.h"

namespace {
using namespace vorta_attn_km;

constexpr int DSS = QSL * 2 + 16;  // bytes per key row of a wave's dS image (the pad spreads the rows over the banks)
// what the key sweep reads comes first: every read there is ONE lane-constant base register plus an immediate
constexpr int DS_OFF = 0;                         // [4 waves][64 keys][32 queries]
constexpr int K_OFF = DS_OFF + 4 * KVB * DSS;
constexpr int V_OFF = K_OFF + TILE_BYTES;
constexpr int Q_OFF = V_OFF + TILE_BYTES;
constexpr int DO_OFF = Q_OFF + SQB * ROWB;
constexpr int DQ_LDS = DO_OFF + SQB * ROWB;

template <typename T>
__global__ __launch_bounds__(KNT) void attn_bwd_dq_kernel(const KmParams kp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
  const Params& p = kp.p;

  __shared__ __attribute__((aligned(16))) char smem[DQ_LDS];

  int y, head, grp, p0, pend;
  if (!q_block_work(kp, y, head, grp, p0, pend)) return;
  const int q_valid = p.q_valid_dev ? min(*p.q_valid_dev, p.q_valid) : p.q_valid;
  pend = min(pend, p.n_q);
  if (p0 >= pend || p0 >= q_valid) return;  // (workgroup-uniform) no position of this block takes a gradient

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r32 = lane & 31;
  const int hh = lane >> 5;

  const int n_kv = p.n_kv_dev ? max(1, min(*p.n_kv_dev, p.n_kv)) : p.n_kv;
  const int nblk = (n_kv + KVB - 1) / KVB;
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)y * p.q_rows_sh : nullptr;

  load_q_images<T>(kp, smem, Q_OFF, DO_OFF, y, head, q_rows, p0, pend, q_valid);
  __syncthreads();
  V8 qf[8], gf[8];
  q_frags<T>(smem, Q_OFF, DO_OFF, wave, qf, gf);

  // ---- the statistics of this lane's 16 queries: register i of an accumulator = query acc_row(i, hh) of the wave
  // (a position that takes no gradient: lse2 = 1e30, so that P = exp2(.. - 1e30) = 0) ----
  const float* st = kp.stats + (int64_t)y * kp.stats_sh;
  float lse2[16], delta[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int pos = p0 + wave * 32 + acc_row(i, hh);
    float2 sd = make_float2(1e30f, 0.f);
    if (pos < pend && pos < q_valid) sd = *(const float2*)(st + 2 * (int64_t)pos);
    lse2[i] = sd.x; delta[i] = sd.y;
  }

  const int32_t* kv_rows =
      p.kv_rows ? p.kv_rows + (int64_t)y * p.kv_rows_sh + (int64_t)grp * p.kv_rows_sg : nullptr;
  KvLoader kv(p, kv_rows, head, n_kv);
  int k_rd[8];
  frag_bases(k_rd);

  // transposed reads (attn_bwd_kmajor.h tr_row): the same k order on both operands of the dQ product
  int ktr[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ktr[h][dt] = K_OFF + tile_off(tr_row() + 8 * h, 32 * dt + tr_col());
  const int dtr = DS_OFF + (wave * KVB + tr_row()) * DSS + tr_col() * 2;
  // the [key][query] image of dS: this lane's key row, queries 4 hh + 0..3 of every group of eight
  char* const srow = smem + DS_OFF + (wave * KVB + r32) * DSS + hh * 8;

  const float c = p.scale_log2;

  f32x16 dq[4];  // [32 channels]: rows = this wave's queries, this lane's column = channel 32 dt + r32
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[dt][i] = 0.f;

  // ---- the key sweep ----
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
    for (int rg = 0; rg < 4; ++rg) {
      V4 x0, x1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * rg + j;
        const float p0v = dead0 ? 0.f : expo(s0[i], c, lse2[i]);
        const float p1v = dead1 ? 0.f : expo(s1[i], c, lse2[i]);
        x0[j] = (T)(p0v * (g0[i] - delta[i]));
        x1[j] = (T)(p1v * (g1[i] - delta[i]));
      }
      *(V4*)(srow + 16 * rg) = x0;
      *(V4*)(srow + 32 * DSS + 16 * rg) = x1;
    }
    // the image is this wave's own: its LDS operations complete in order, so the reads below see the stores above
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // dQ[q][32 dt + r32] += dS . K over the block's 64 keys
#pragma unroll
    for (int kk = 0; kk < KVB / 16; ++kk) {
      const V4 lo = MF<T>::tr(smem + dtr + 16 * kk * DSS), hi = MF<T>::tr(smem + dtr + (16 * kk + 8) * DSS);
      V8 xs;
#pragma unroll
      for (int j = 0; j < 4; ++j) { xs[j] = lo[j]; xs[4 + j] = hi[j]; }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const V4 lo2 = MF<T>::tr(smem + ktr[0][dt] + 16 * kk * ROWB), hi2 = MF<T>::tr(smem + ktr[1][dt] + 16 * kk * ROWB);
        V8 xk;
#pragma unroll
        for (int j = 0; j < 4; ++j) { xk[j] = lo2[j]; xk[4 + j] = hi2[j]; }
        dq[dt] = MF<T>::mfma(xs, xk, dq[dt]);
      }
    }
    __syncthreads();  // every wave is done with the K / V tiles
  }

  // ---- epilogue: dq[r(p)] += scale dQ (one writer per row) ----
  float* dqh = kp.dq + (int64_t)head * kp.dq_sh + r32;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int pos = p0 + wave * 32 + acc_row(i, hh);
    if (pos < pend && pos < q_valid) {
      const int64_t row = q_rows ? (int64_t)q_rows[pos] : (int64_t)(p.q_row_offset + pos);
      float* dst = dqh + row * kp.dq_ss;
      float old[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) old[dt] = dst[32 * dt];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dst[32 * dt] = old[dt] + dq[dt][i] * kp.scale;
    }
  }
#endif
}

}  // namespace

extern "C" int vorta_attn_bwd_dq(const vorta_attn_bwd_kmajor_args* a, void* hip_stream) {
  KmParams kp{};
  const int rc = fill_km(a, kp, false);
  if (rc != VORTA_OK) return rc;
  if (!f32_rows_ok(a->bwd.dq)) return VORTA_EINVAL;  // (dk / dv are not looked at)
  const Params& p = kp.p;
  if (p.n_heads == 0) return VORTA_OK;
  return launch_km(a, attn_bwd_dq_kernel<__bf16>, attn_bwd_dq_kernel<_Float16>, (int64_t)p.wg_per_slot * p.n_heads, hip_stream,
                   kp);
}
