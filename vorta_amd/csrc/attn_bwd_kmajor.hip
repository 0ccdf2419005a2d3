// KEY-MAJOR gather flash-attention backward for gfx950 (MI355X, CDNA4): include/vorta_hip.h vorta_attn_bwd_kmajor.  The same
// gradient as vorta_attn_bwd (csrc/attn_bwd.hip), organised around the keys: the query-major kernel adds a dK and a dV tile
// with float atomics for EVERY (query block, key block) pair and runs at the chip's atomic rate; here a workgroup owns 256
// keys and keeps their dK and dV on chip for the whole query sweep, and only dQ -- a quarter of the bytes per pair at this tile
// shape, 16 KiB per (32 queries x 256 keys) -- crosses workgroups.  It needs the softmax statistics of every query row before it
// starts: vorta_attn_bwd_stats (csrc/attn_bwd_stats.hip) writes them.
//
// One workgroup (4 waves) = one 256-key block of one (head slot, group) key list; wave w keeps keys 64 w .. 64 w + 63.  It
// sweeps the query positions of THAT group in 32-row slices (with a q_block_table: every table row of the group, found by
// scanning the table).  The sweep's pieces -- the K image, the V fragments, the slice loader, the S / dP / P / dS step and the
// dV / dK products -- are the KEY-BLOCK SWEEP section of csrc/attn_bwd_kmajor.h, shared with csrc/attn_bwd_dkv.hip.  Per slice:
//     S = Q . K^T, dP = dO_eff . V^T      P = exp2(c s - lse2)      dS = P (dP - delta)             (sweep_scores)
//     dV[key][d] += P^T . dO_eff          dK[key][d] += dS^T . Q                                    (sweep_dkv)
//     dS goes to LDS once, 16 bits, as a [key][query] image; after a barrier every wave takes 32 channels of
//     dQ_slice[q][d] = sum over all 256 keys of dS[q][key] K[key][d]    (the sum over the four waves is the MFMA's own)
//     and adds scale dQ_slice to the fp32 dq rows with vector float atomics (global_atomic_add_f32): one register of the
//     32 x 32 accumulator is two 128-byte row segments per wave-instruction.
// At the end of the sweep the workgroup adds scale dK and dV to the fp32 dk / dv rows, with the same atomics in the same
// shape: key lists of different groups overlap (sliding tile) and the three experts of the mixture share the buffers.
// K stays in LDS for the whole sweep (64 KiB, row reads for S and transposed reads for dQ), V in registers (it is only ever
// the B operand of dP).  The next slice's q, d_o and statistics rows are loaded one slice ahead.
//
// REPRODUCIBILITY: none of dq, dk, dv is bit-reproducible from run to run (the summation order of float atomics).  There is
// no protocol between workgroups of any kind -- no ordered hand-off, no tickets, no waiting on memory: a workgroup never
// depends on another one's progress.
// LDS: K 64 K + Q 8 K + dO_eff 8 K + dS 20 K + statistics and row numbers < 1 K = 101 KiB: one workgroup per CU (as the
// 512 registers per lane already make it).
// Registers: dK and dV fill the 256 accumulator registers, so the S / dP / dQ accumulators must live in the other 256.  The
// compiler's default gives EVERY MFMA of a kernel that uses accumulator registers an accumulator-register result and spills
// (792 B of scratch); vorta_amd/build.py compiles this file with -mllvm -amdgpu-mfma-vgpr-form, which lets the register
// allocator choose per value: no scratch, no spill.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_bwd_kmajor.h"

namespace {
using namespace vorta_attn_km;

constexpr int DSS = QSL * 2 + 16;  // bytes per key row of the dS image (the pad spreads the rows over the banks)
// the small images first: every read below is ONE lane-constant base register plus an immediate (16 bits reach 64 KiB)
constexpr int DS_OFF = SL_DO + QSL * ROWB;     // (the slice buffer -- Q, dO_eff -- is at 0)
constexpr int ST_OFF = DS_OFF + KMB * DSS;     // [32] (lse2, delta)
constexpr int ROW_OFF = ST_OFF + QSL * 8;      // [2][32] int64 dq row of a slice's position, -1 = none (two slices in flight)
constexpr int K_OFF = ROW_OFF + 2 * QSL * 8;
constexpr int KM_LDS = K_OFF + KMB * ROWB;

template <typename T>
__global__ __launch_bounds__(KNT) void attn_bwd_kmajor_kernel(const KmParams kp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
  const Params& p = kp.p;

  __shared__ __attribute__((aligned(16))) char smem[KM_LDS];

  // ---- work decomposition: (head slot, group, key block) ----
  const int wg = live_order(p, blockIdx.x, gridDim.x, p.xcd_remap);
  const int kb = wg % kp.n_kblocks;
  const int grp = (wg / kp.n_kblocks) % kp.n_lists;
  const int y = wg / (kp.n_kblocks * kp.n_lists);
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
  SliceLoader<T, true> ld(kp, q_rows, y, head, w);

  const SweepBases lb(wave, K_OFF);
  const int d0 = 32 * wave;  // dQ: this wave's channels
  int ktr[2];                // transposed reads of the K image (attn_bwd_kmajor.h tr_row), as lane-constant as lb's
#pragma unroll
  for (int h = 0; h < 2; ++h) ktr[h] = K_OFF + tile_off(tr_row() + 8 * h, d0 + tr_col());
  const int dtr = DS_OFF + tr_row() * DSS + tr_col() * 2;
  const int strd = ST_OFF + 4 * hh * 8;

  f32x16 dk[2][4], dv[2][4];  // [key half][32 channels]: rows = the half's keys, this lane's column = channel 32 dt + r32
#pragma unroll
  for (int kh = 0; kh < 2; ++kh)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dk[kh][dt][i] = 0.f; dv[kh][dt][i] = 0.f; }

  ld.issue(sl_p0, sl_end);
  ld.write(smem, sl_p0, sl_end, 0, ST_OFF, ROW_OFF);
  float* dqh = kp.dq + (int64_t)head * kp.dq_sh + d0 + r32;

  bool have = true;
  for (int it = 0; have; ++it) {
    __syncthreads();  // this slice's images are in place (first turn: the K image too); the dS image is free
    int nx_r = sl_r, nx_p0 = sl_p0, nx_end = sl_end;
    const bool have_next = next_slice(kp, grp, q_valid, nx_r, nx_p0, nx_end);
    if (have_next) ld.issue(nx_p0, nx_end);

#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const bool dead = kb * KMB + key0 + 32 * kh >= n_kv;  // (the tail of the last key block)
      V8 pb[2], dsb[2];
      sweep_scores<T>(smem, smem, lb, kh, vf[kh], strd, dead, c, pb, dsb);
      // the [key][query] image of dS: register group rg holds queries 8 rg + 4 hh + 0..3 of this lane's key
      char* srow = smem + DS_OFF + (key0 + 32 * kh) * DSS + hh * 8;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        V4 x;
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = dsb[rg >> 1][4 * (rg & 1) + j];
        *(V4*)(srow + 16 * rg) = x;
      }
      sweep_dkv<T>(smem, lb, pb, dsb, dv[kh], dk[kh]);
    }
    __syncthreads();  // the dS image is complete; every wave is done with the Q / dO_eff images and the statistics
    if (have_next) ld.write(smem, nx_p0, nx_end, 0, ST_OFF, ROW_OFF + ((it + 1) & 1) * QSL * 8);

    // dQ_slice[q][d0 + r32] over all 256 keys
    {
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int kk = 0; kk < KMB / 16; ++kk) {
        const V4 lo = MF<T>::tr(smem + dtr + 16 * kk * DSS), hi = MF<T>::tr(smem + dtr + (16 * kk + 8) * DSS);
        const V4 lo2 = MF<T>::tr(smem + ktr[0] + 16 * kk * ROWB), hi2 = MF<T>::tr(smem + ktr[1] + 16 * kk * ROWB);
        V8 xs, xk;
#pragma unroll
        for (int j = 0; j < 4; ++j) { xs[j] = lo[j]; xs[4 + j] = hi[j]; xk[j] = lo2[j]; xk[4 + j] = hi2[j]; }
        acc = MF<T>::mfma(xs, xk, acc);
      }
      const char* rows = smem + ROW_OFF + (it & 1) * QSL * 8 + 4 * hh * 8;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t row = *(const int64_t*)(rows + acc_row(i, 0) * 8);
        if (row >= 0) unsafeAtomicAdd(dqh + row * kp.dq_ss, acc[i] * kp.scale);
      }
    }
    have = have_next;
    sl_r = nx_r; sl_p0 = nx_p0; sl_end = nx_end;
  }

  // ---- epilogue: dk[row(key)] += scale dK, dv[row(key)] += dV ----
  float* dvh = kp.dv + (int64_t)head * kp.dv_sh + r32;
  float* dkh = kp.dk + (int64_t)head * kp.dk_sh + r32;
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pos = kb * KMB + wave * 64 + 32 * kh + acc_row(i, hh);
      if (pos < n_kv) {
        const int64_t row = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          unsafeAtomicAdd(dvh + row * kp.dv_ss + 32 * dt, dv[kh][dt][i]);
          unsafeAtomicAdd(dkh + row * kp.dk_ss + 32 * dt, dk[kh][dt][i] * kp.scale);
        }
      }
    }
  }
#endif
}

}  // namespace

extern "C" int vorta_attn_bwd_kmajor(const vorta_attn_bwd_kmajor_args* a, void* hip_stream) {
  KmParams kp{};
  const int rc = fill_km(a, kp, true);
  if (rc != VORTA_OK) return rc;
  Params& p = kp.p;
  if (p.n_heads == 0) return VORTA_OK;
  p.wg_per_slot = kp.n_lists * kp.n_kblocks;  // this kernel's workgroups per head slot (live_order)
  return launch_km(a, attn_bwd_kmajor_kernel<__bf16>, attn_bwd_kmajor_kernel<_Float16>, (int64_t)p.wg_per_slot * p.n_heads,
                   hip_stream, kp);
}

extern "C" int vorta_attn_bwd_kmajor_args_size(void) { return (int)sizeof(vorta_attn_bwd_kmajor_args); }
