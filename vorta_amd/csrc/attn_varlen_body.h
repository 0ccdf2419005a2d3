// The body of the 16-bit attention launches whose query groups walk key lists of DIFFERENT lengths (attn_fwd_varlen.hip: the
// lists are rows of a kv_rows table; attn_fwd_tilelist.hip: the lists are TILE lists, read through one tile-major row table).
// One arithmetic, so the two launches write the same bits for the same rows; only where a key row id comes from differs, and
// that is the body's `Rows` policy:
//   Rows::LDS_BYTES                       LDS the policy keeps behind the body's K and V rings
//   Rows(src, p, w, lds, wave, lane)      built by every thread of the workgroup once decode_work has let it in (it may hold a
//                                         workgroup barrier); `src` is the launch's own parameter block
//   rows.len                              the group's list length: workgroup-uniform, at least 1
//   rows.fetch(blk, rowN)                 the row ids of the lane's CH DMA pieces of key block blk -- positions blk * 64 +
//                                         4 (CH wave + i) + lane / 16 -- every position clamped to len - 1.  The body calls it
//                                         for blk = 0, 1, 2, ... in that order, one block ahead of the DMA request
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"

namespace vorta_attn {

constexpr int NSV = 2;  // ring depth of the K and of the V tiles: 64 KiB of LDS

template <int NW> constexpr int varlen_pieces = (KVB * 16) / (NW * 64);  // 1-KiB DMA pieces (4 tile rows) of one tile per wave (2 or 4)

template <typename T, int NW, class Rows, class PP>
__device__ __forceinline__ void attn_varlen_body(const PP& pp, char* __restrict__ smem, const int wg) {
  const Params& p = pp.p;
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
  constexpr int QB = NW * 32;
  constexpr int CH = varlen_pieces<NW>;
  Work w;
  if (!decode_work<QB>(p, wg, w)) return;
  const int head = w.head;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the group's own length: uniform, so it lives in a scalar register and the loop bound is one
  Rows rows(pp, p, w, smem + 2 * NSV * TILE_BYTES, wave, lane);
  const int len = rows.len;
  // a workgroup whose rows are all past q_valid has no key loop: its rows are zero bits whatever the keys hold
  const int nblk = w.p0 >= w.q_valid ? 0 : (len + KVB - 1) / KVB;

  const int r32 = lane & 31;
  const int hh = lane >> 5;

  // ---- query rows ----
  const int wrow0 = w.p0 + wave * 32;
  const bool wave_active = wrow0 < w.pend;  // wave-uniform
  // a wave whose rows are all past q_valid requests tiles and meets the barriers, computes nothing and writes zero rows
  const bool wave_compute = wave_active && wrow0 < w.q_valid;
  const int64_t my_row = q_row_of(p, w, wrow0 + r32);
  V8 qf[8];
  {
    const char* qp = p.q + (int64_t)head * p.q_sh + my_row * p.q_ss + hh * 16;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const V8 raw = *(const V8*)(qp + ks * 32);
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[ks][i] = (T)((float)raw[i] * p.scale_log2);
    }
  }

  // ---- loader: a wave instruction fills 1 KiB = 4 tile rows; the lane that lands in chunk c' of row r fetches chunk
  // c' ^ swz(r) of that row (the involution the fragment reads apply) ----
  const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.k + (int64_t)head * p.k_sh), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.v + (int64_t)head * p.v_sh), 0, 0x7fffffff, 0x00020000);
  const int k_ss32 = (int)p.k_ss, v_ss32 = (int)p.v_ss;
  int k_col[CH], v_col[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int row = 4 * (CH * wave + i) + (lane >> 4);
    k_col[i] = ((lane & 15) ^ (row & 15)) << 4;
    v_col[i] = ((lane & 15) ^ ((row & 3) << 2)) << 4;
  }
  int rowN[CH];  // row ids of the next block to request, fetched a step ahead of the request
#define ROWS_OF(blk_) rows.fetch((blk_), rowN);
#define DMA_KV(slot_)                                                             \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) {                             \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(k_rsrc, (LDS_AS void*)(smem + (slot_) * TILE_BYTES + (CH * wave + i_) * 1024), 16, \
        (int)__umul24((unsigned)rowN[i_], (unsigned)k_ss32) + k_col[i_], 0, 0, 0); \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(v_rsrc, (LDS_AS void*)(smem + (NSV + (slot_)) * TILE_BYTES + (CH * wave + i_) * 1024), 16, \
        (int)__umul24((unsigned)rowN[i_], (unsigned)v_ss32) + v_col[i_], 0, 0, 0); \
  }
  // end of a step: own requests have landed, then the workgroup barrier (which also orders every wave's reads of this
  // step before the next step's overwrites)
#define STEP_SYNC() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");

  // ---- LDS read addresses ----
  int k_rd[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) k_rd[ks] = r32 * ROWB + (((2 * ks + hh) ^ (r32 & 15)) << 4);
  int v_rd[4];
  {
    const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, c4 = i16 & 3;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      v_rd[dt] = NSV * TILE_BYTES + (4 * (g >> 1) + q4) * ROWB + ((dt ^ q4) << 6) + 32 * (g & 1) + 8 * c4;
  }

  f32x16 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  // online softmax in the exp2 domain: m_run = the row's reference point (at most `defer` below its running max), the
  // score MFMAs start from minit = -m_run, so they deliver z - m_run and P = exp2 of that
  float m_run = 0.f, l_run = 0.f;
  const float defer = p.defer_log2;
  f32x16 minit;
#pragma unroll
  for (int i = 0; i < 16; ++i) minit[i] = 0.f;

  // Issue order of the two matrix phases (sched_group_barrier: 0x008 MFMA, 0x100 DS read): a fragment read per score MFMA,
  // the two transposed V reads per P V MFMA.  Left to itself the scheduler lifts every fragment read of a phase in front of
  // its first MFMA: 64 + 64 registers of fragments on top of the accumulators, and the allocator spills.
#define SCHED_QK()                                                                \
  _Pragma("unroll") for (int g_ = 0; g_ < 16; ++g_) {                             \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                            \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                            \
  }
#define SCHED_PV()                                                                \
  _Pragma("unroll") for (int g_ = 0; g_ < 16; ++g_) {                             \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                            \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                            \
  }
  // one key block j, its tiles in ring slot cur_
#define STEP(cur_, j_)                                                            \
  {                                                                               \
    if ((j_) + 1 < nblk) {                                                        \
      DMA_KV((cur_) ^ 1)                                                          \
      ROWS_OF((j_) + 2)                                                           \
    }                                                                             \
    if (wave_compute) {                                                           \
      f32x16 s0_, s1_;                                                            \
      _Pragma("unroll") for (int ks_ = 0; ks_ < 8; ++ks_) {                       \
        const V8 k0_ = *(const V8*)(smem + (cur_) * TILE_BYTES + k_rd[ks_]);      \
        const V8 k1_ = *(const V8*)(smem + (cur_) * TILE_BYTES + k_rd[ks_] + 32 * ROWB); \
        s0_ = MF<T>::mfma(k0_, qf[ks_], ks_ == 0 ? minit : s0_);                  \
        s1_ = MF<T>::mfma(k1_, qf[ks_], ks_ == 0 ? minit : s1_);                  \
      }                                                                           \
      SCHED_QK()                                                                  \
      if ((j_) * KVB + KVB > len) { /* the tail of the group's list */            \
        int h4_ = 4 * hh; /* opaque: else the 16 sums lane term + register row are hoisted into 16 registers */ \
        asm volatile("" : "+v"(h4_));                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) {                       \
          const int row_ = (i_ & 3) + 8 * (i_ >> 2) + h4_;                        \
          if ((j_) * KVB + row_ >= len) s0_[i_] = -INFINITY;                      \
          if ((j_) * KVB + 32 + row_ >= len) s1_[i_] = -INFINITY;                 \
        }                                                                         \
      }                                                                           \
      float mx_ = s0_[0];                                                         \
      _Pragma("unroll") for (int i_ = 1; i_ < 16; ++i_) mx_ = fmaxf(mx_, s0_[i_]); \
      _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) mx_ = fmaxf(mx_, s1_[i_]); \
      mx_ = half_max(mx_);                                                        \
      /* deferred rescale: the reference point moves when some row of the wave outgrew it by more than `defer`; rows */ \
      /* that did not grow keep theirs (g = 0).  The first block fixes it at the block's true row max (it always     */ \
      /* holds a listed key; O and l are zero there, so alpha = 0 stands for any factor)                             */ \
      if ((j_) == 0 || !__all(mx_ <= defer)) {                                    \
        const float g_ = (j_) == 0 ? mx_ : fmaxf(mx_, 0.f);                       \
        const float alpha_ = (j_) == 0 ? 0.f : __builtin_amdgcn_exp2f(-g_);       \
        _Pragma("unroll") for (int dt_ = 0; dt_ < 4; ++dt_)                       \
          _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) o[dt_][i_] *= alpha_; \
        l_run *= alpha_;                                                          \
        m_run += g_;                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) { s0_[i_] -= g_; s1_[i_] -= g_; minit[i_] = -m_run; } \
        asm volatile("" : "+v"(minit));                                           \
      }                                                                           \
      float lsum_ = 0.f;                                                          \
      _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) {                         \
        s0_[i_] = __builtin_amdgcn_exp2f(s0_[i_]);                                \
        s1_[i_] = __builtin_amdgcn_exp2f(s1_[i_]);                                \
        lsum_ += s0_[i_] + s1_[i_];                                               \
      }                                                                           \
      l_run += lsum_;                                                             \
      V8 pb_[4];                                                                  \
      _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                          \
        pb_[0][e_] = (T)s0_[e_];                                                  \
        pb_[1][e_] = (T)s0_[8 + e_];                                              \
        pb_[2][e_] = (T)s1_[e_];                                                  \
        pb_[3][e_] = (T)s1_[8 + e_];                                              \
      }                                                                           \
      _Pragma("unroll") for (int dt_ = 0; dt_ < 4; ++dt_) {                       \
        _Pragma("unroll") for (int kg_ = 0; kg_ < 4; ++kg_) {                     \
          const V4 lo_ = MF<T>::tr(smem + (cur_) * TILE_BYTES + v_rd[dt_] + (16 * kg_) * ROWB); \
          const V4 hi_ = MF<T>::tr(smem + (cur_) * TILE_BYTES + v_rd[dt_] + (16 * kg_ + 8) * ROWB); \
          V8 vf_;                                                                 \
          _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) { vf_[e_] = lo_[e_]; vf_[4 + e_] = hi_[e_]; } \
          o[dt_] = MF<T>::mfma(vf_, pb_[kg_], o[dt_]);                            \
        }                                                                         \
      }                                                                           \
      SCHED_PV()                                                                  \
    }                                                                             \
    STEP_SYNC()                                                                   \
  }

  if (nblk > 0) {
    ROWS_OF(0)
    DMA_KV(0)
    ROWS_OF(1)
    STEP_SYNC()
  }
  for (int j = 0; j < nblk; j += 2) {
    STEP(0, j)
    if (j + 1 >= nblk) break;
    STEP(1, j + 1)
  }
#undef STEP
#undef STEP_SYNC
#undef SCHED_QK
#undef SCHED_PV
#undef DMA_KV
#undef ROWS_OF

  if (!wave_active) return;
  write_rows<T>(p, w, wrow0, o, m_run, half_sum(l_run));
}

}  // namespace vorta_attn
