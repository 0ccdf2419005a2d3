// Gather flash-attention forward whose query groups have key lists of DIFFERENT lengths, for gfx950 (MI355X, CDNA4):
// include/vorta_hip.h vorta_attn_fwd_varlen.  16 bits (bf16 / fp16), D = 128, a kv_rows table required.
//
// vorta_attn_fwd walks one n_kv per launch.  Here group g of head slot y attends the first kv_len[y][g] entries of its list
// and nothing behind them: the sliding-tile expert under sliding_keys="share" keeps a different number of key tiles per
// (head, query tile) (sta_share.hip), and a workgroup's key loop is as long as its own list.
//
// The body is built on the two shared ends of attn_common.h (decode_work, write_rows) and on the family's 32x32x16 scheme:
//   * swapped product S^T[kv][q] = K . Q^T: a lane owns one query and 16 + 16 of a block's 64 scores; the accumulator is the
//     B operand of O^T[d][q] = V^T . P^T as it stands;
//   * Q pre-multiplied by scale log2(e) and re-rounded, the score MFMAs seeded with minus the row's reference point, the
//     reference moved only when a row outgrows it by more than `defer` binades: the arithmetic of attn_pipe_dma_body;
//   * K tile with the 16-way XOR swizzle, V tile with the 64-byte-quadrant swizzle read through ds_read_b64_tr_b16; both
//     staged global -> LDS by DMA (the swizzle applied on the source side), rings of 2, 64-key blocks, ONE barrier a block.
// What is new:
//   * the group's length is a scalar: one load through a workgroup-uniform address, in readfirstlane form, clamped into
//     [1, n_kv].  It bounds the key loop and every row-id fetch (positions are clamped to len - 1, so no entry behind the
//     length is read and a tail block's spare rows are copies of the last listed key);
//   * a tail block (len not a multiple of 64) is masked as the table body masks it: -inf into the scores past len;
//   * the logical workgroup comes through `order` (physical block b computes order[b]): key loops of one launch differ by up
//     to n_sel x, and a grid dealt in index order ends with whichever long loops came last.  sta_share.hip writes the order
//     longest first.  NULL: the XCD-aware index order of the family.  (attn_common.h varlen_workgroup; the tables and the
//     host checks of vorta_attn_varlen_ext are its VarTables / fill_var_tables, shared with attn_fwd_i8_varlen.hip.)
// The step is simpler than attn_pipe_dma_body's: scores, softmax and P V of block j in step j (no scores one block ahead),
// K(j+1) and V(j+1) requested at the top of step j into the slots step j-1 read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"

namespace {
using namespace vorta_attn;

struct ParamsVar {
  Params p;
  VarTables t;
};

constexpr int NSV = 2;  // ring depth of the K and of the V tiles: 64 KiB of LDS

template <typename T, int NW>
__device__ __forceinline__ void attn_varlen_body(const ParamsVar& pp, char* __restrict__ smem, const int wg) {
  const Params& p = pp.p;
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
  constexpr int NT = NW * 64;
  constexpr int QB = NW * 32;
  constexpr int CH = (KVB * 16) / NT;  // 1-KiB DMA pieces (4 tile rows) of one tile per wave (2 or 4)
  Work w;
  if (!decode_work<QB>(p, wg, w)) return;
  const int y = w.y, head = w.head, grp = w.grp;
  // the group's own length: uniform, so it lives in a scalar register and the loop bound is one
  const int len = max(1, min(__builtin_amdgcn_readfirstlane(pp.t.kv_len[(int64_t)y * pp.t.kv_len_sh + grp]), w.n_kv));
  // a workgroup whose rows are all past q_valid has no key loop: its rows are zero bits whatever the keys hold
  const int nblk = w.p0 >= w.q_valid ? 0 : (len + KVB - 1) / KVB;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  const int32_t* kv_rows = p.kv_rows + (int64_t)y * p.kv_rows_sh + (int64_t)grp * p.kv_rows_sg;
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
#define ROWS_OF(blk_)                                                             \
  _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_)                               \
    rowN[i_] = kv_rows[min((blk_) * KVB + 4 * (CH * wave + i_) + (lane >> 4), len - 1)];
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

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_varlen_kernel(const ParamsVar pp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  __shared__ __attribute__((aligned(16))) char smem[2 * NSV * TILE_BYTES];
  attn_varlen_body<T, NW>(pp, smem, varlen_workgroup(pp.t, pp.p));
#endif
}

template <typename T>
int launch(const ParamsVar& pp, int block_rows, hipStream_t st) {
  return launch_varlen(attn_varlen_kernel<T, 8>, attn_varlen_kernel<T, 4>, pp.p, pp, block_rows, st);
}

}  // namespace

extern "C" int vorta_attn_varlen_ext_size(void) { return (int)sizeof(vorta_attn_varlen_ext); }

extern "C" int vorta_attn_fwd_varlen(const vorta_attn_args* a, const vorta_attn_varlen_ext* ext, void* hip_stream) {
  if (!varlen_ext_sized(ext)) return VORTA_EINVAL;
  ParamsVar pp{};
  int block_rows = 0;
  int rc = fill_params(a, pp.p, block_rows, 2);  // (a dtype other than bf16 / fp16: VORTA_EUNSUPPORTED there)
  if (rc == VORTA_OK) rc = fill_var_tables(a, ext, pp.p, pp.t);  // (one body: the LDS-DMA one)
  if (rc != VORTA_OK) return rc;
  if (pp.p.n_heads == 0 || pp.p.n_groups == 0) return VORTA_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  return a->dtype == VORTA_BF16 ? launch<__bf16>(pp, block_rows, st) : launch<_Float16>(pp, block_rows, st);
}
