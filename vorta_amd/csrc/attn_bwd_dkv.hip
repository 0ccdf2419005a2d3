// The dK / dV pass of the DETERMINISTIC attention backward for gfx950 (MI355X, CDNA4): include/vorta_hip.h vorta_attn_bwd_dkv.
// The key-major sweep of csrc/attn_bwd_kmajor.hip reduced to what dK and dV need: no dS image, no dQ product, no atomic.  It
// needs the softmax statistics of every query row (vorta_attn_bwd_stats, csrc/attn_bwd_stats.hip); vorta_attn_bwd_dq
// (csrc/attn_bwd_dq.hip) gives dq.
//
// One LAUNCH = one key list (group); one workgroup (4 waves) = one 256-key block of that list for one head slot; wave w keeps
// keys 64 w .. 64 w + 63.  It sweeps the query positions of the group in 32-row slices, in the key-major kernel's order and
// through the same pieces (the KEY-BLOCK SWEEP section of csrc/attn_bwd_kmajor.h: the K image, the V fragments, the slice
// loader, sweep_scores for S / dP / P / dS, sweep_dkv for dV += P^T . dO_eff and dK += dS^T . Q).
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

// two slice buffers first, then the K image (every read is one lane-constant base register, the buffer's offset and an
// immediate)
constexpr int ST_OFF = SL_DO + QSL * ROWB;   // [32] (lse2, delta)
constexpr int SLB = ST_OFF + QSL * 8;        // bytes of a slice buffer (a multiple of 256: the same banks in both)
constexpr int K_OFF = 2 * SLB;
constexpr int DKV_LDS = K_OFF + KMB * ROWB;

template <typename T>
__global__ __launch_bounds__(KNT) void attn_bwd_dkv_kernel(const KmParams kp, const int grp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  using V8 = typename MF<T>::v8;
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

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r32 = lane & 31;
  const int hh = lane >> 5;
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)y * p.q_rows_sh : nullptr;
  const int32_t* kv_rows =
      p.kv_rows ? p.kv_rows + (int64_t)y * p.kv_rows_sh + (int64_t)grp * p.kv_rows_sg : nullptr;
  const float c = p.scale_log2;
  float w = 1.f;
  if (kp.do_scale) w = (float)((const T*)kp.do_scale)[(int64_t)head * kp.do_scale_sh];

  load_k_image(p, smem, K_OFF, kv_rows, head, kb, n_kv);
  const int key0 = wave * 64 + r32;  // this lane's row of the K image; its second key is 32 rows on
  V8 vf[2][8];
  load_v_frags<T>(p, kv_rows, head, kb * KMB + key0, n_kv, vf);
  SliceLoader<T, false> ld(kp, q_rows, y, head, w);
  const SweepBases lb(wave, K_OFF);
  const int strd = ST_OFF + 4 * hh * 8;

  f32x16 dk[2][4], dv[2][4];  // [key half][32 channels]: rows = the half's keys, this lane's column = channel 32 dt + r32
#pragma unroll
  for (int kh = 0; kh < 2; ++kh)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dk[kh][dt][i] = 0.f; dv[kh][dt][i] = 0.f; }

  ld.issue(sl_p0, sl_end);
  ld.write(smem, sl_p0, sl_end, 0, ST_OFF);

  bool have = true;
  for (int it = 0; have; ++it) {
    // this slice's images are in place (first turn: the K image too), and every wave is done with the other buffer, which it
    // read a turn ago
    __syncthreads();
    const int cur = (it & 1) * SLB;
    const char* sb = smem + cur;
    int nx_r = sl_r, nx_p0 = sl_p0, nx_end = sl_end;
    const bool have_next = next_slice(kp, grp, q_valid, nx_r, nx_p0, nx_end);
    if (have_next) ld.issue(nx_p0, nx_end);

#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const bool dead = kb * KMB + key0 + 32 * kh >= n_kv;  // (the tail of the last key block)
      // (no instruction) no LDS store separates the two halves here, and the compiler would keep the first half's Q / dO_eff
      // fragments and statistics for the second: 64 + 32 registers the accumulators have taken, 93 spilled.  Read them again.
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      V8 pb[2], dsb[2];
      sweep_scores<T>(smem, sb, lb, kh, vf[kh], strd, dead, c, pb, dsb);
      sweep_dkv<T>(sb, lb, pb, dsb, dv[kh], dk[kh]);
    }
    if (have_next) ld.write(smem, nx_p0, nx_end, SLB - cur, ST_OFF);
    have = have_next;
    sl_r = nx_r; sl_p0 = nx_p0; sl_end = nx_end;
  }

  // ---- epilogue: dk[row(key)] += scale dK, dv[row(key)] += dV (this workgroup is the rows' only writer in the launch) ----
  float* dvh = kp.dv + (int64_t)head * kp.dv_sh + r32;
  float* dkh = kp.dk + (int64_t)head * kp.dk_sh + r32;
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pos = kb * KMB + wave * 64 + 32 * kh + acc_row(i, hh);
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
  // one launch per key list, in list order: rows that two lists share are added to list by list
  for (int grp = 0; grp < kp.n_lists; ++grp) {
    const int lrc = launch_km(a, attn_bwd_dkv_kernel<__bf16>, attn_bwd_dkv_kernel<_Float16>, (int64_t)p.wg_per_slot * p.n_heads,
                              hip_stream, kp, grp);
    if (lrc != VORTA_OK) return lrc;
  }
  return VORTA_OK;
}
