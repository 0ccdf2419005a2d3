// Gather flash-attention BACKWARD for gfx950 (MI355X, CDNA4): include/vorta_hip.h vorta_attn_bwd.  The gradient of exactly
// what one vorta_attn_fwd launch computes, for the same argument block: one kernel serves the dense, coreset and sliding-tile
// experts, which differ only in their row tables.
//
// Query-major like the forward: a workgroup (4 waves) owns one block of 128 query positions of one (head slot, group) and
// walks the group's key list in 64-key blocks, twice:
//   pass 1   S^T = K . Q^T and dP^T = V . dO^T: the row maximum m and the row sum l of the softmax (the forward keeps
//            neither) and delta = sum_j P_j dP_j.  In exact arithmetic that is dO_eff . o, the usual form; taken from
//            the SAME P and dP that pass 2 forms, sum_j dS_j cancels to rounding of these very numbers, and a row with one
//            key (P = 1) gets dS = 0 exactly, as float64 autograd does -- dO_eff . o leaves a 1e-7 residue there, because
//            an MFMA and a VALU dot product do not add in the same order;
//   pass 2   phase A, every wave on its own 32 queries, in the forward's operand layouts (a lane owns ONE query):
//              S^T = K . Q^T, dP^T = V . dO^T, P = exp2(c (s - m)) / l, dS = P (dP - delta), dQ^T += K^T . dS^T
//              (dQ stays in accumulators); P and dS are rounded to 16 bits and written to LDS as [query][key] images;
//            phase B, the workgroup together: the sums over ALL 128 queries
//              dV[key][d] = sum_q P[q][key] dO[q][d],   dK[key][d] = scale sum_q dS[q][key] Q[q][d]
//            are 16 tiles of 32 x 32, four per wave (its 32 channels, both key halves, dK and dV); both operands come out
//            of LDS through transposed reads (ds_read_b64_tr_b16), and the tile is ADDED to the fp32 dk / dv buffers with
//            vector float atomics (global_atomic_add_f32): many query blocks touch one key row.  dK / dV are therefore not
//            bit-reproducible from run to run (summation order); dQ is (plain read-add-write, one writer per row).
// The prologue builds, once per query block, the LDS images of Q and of
//     dO_eff[p] = w[head] (dO[r(p)] + sum_i dO[dup_rows[p][i]])      (zero for p >= q_valid: the forward wrote zeros there)
// (fwd.o is validated but not read, see pass 1).  Every LDS tile is row-major with 256-byte rows and the forward's 16-way XOR swizzle of
// the K tile; the same image serves the ds_read_b128 fragment reads and the transposed reads.
// LDS: Q 32 K + dO 32 K + K 16 K + V 16 K + P 18 K + dS 18 K = 132 KiB: one workgroup per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

#include "attn_common.h"

namespace {
using namespace vorta_attn;

constexpr int BNW = 4;                 // waves per workgroup
constexpr int BQB = BNW * 32;          // query rows per workgroup
constexpr int BNT = BNW * 64;          // threads
constexpr int PSTRIDE = KVB * 2 + 16;  // bytes per query row of the P / dS images (the pad spreads the rows over the banks)
constexpr int Q_OFF = 0;
constexpr int DO_OFF = Q_OFF + BQB * ROWB;
constexpr int K_OFF = DO_OFF + BQB * ROWB;
constexpr int V_OFF = K_OFF + TILE_BYTES;
constexpr int P_OFF = V_OFF + TILE_BYTES;
constexpr int DS_OFF = P_OFF + BQB * PSTRIDE;
constexpr int BWD_LDS = DS_OFF + BQB * PSTRIDE;

struct BwdParams {
  Params p;             // the forward launch
  const char* d_o; int64_t do_sh, do_ss;  // bytes
  const void* do_scale; int64_t do_scale_sh;  // elements
  float* dq; float* dk; float* dv;
  int64_t dq_sh, dq_ss, dk_sh, dk_ss, dv_sh, dv_ss;  // floats
  float scale;
  int sub;              // with a q_block_table: 128-row workgroups per table row
};

// byte offset of 16-bit element (row, ecol) of a 256-byte-row tile: 16-byte chunks XOR-swizzled with the row (the forward's K tile)
__device__ __forceinline__ int tile_off(int row, int ecol) {
  const int bc = ecol * 2;
  return row * ROWB + (((bc >> 4) ^ (row & 15)) << 4) + (bc & 15);
}

// exponent of a probability, exp2(s c - mc): the product is rounded BEFORE the subtraction (no fused multiply-add -- the
// rounding functions of the HIP headers are plain operators and would be contracted), so a row's maximum gives exp2(0) = 1
// exactly and the same bits in both passes
__device__ __forceinline__ float rounded_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float expo(float s, float c, float mc) {
#pragma clang fp contract(off)
  const float t = s * c;
  return __builtin_amdgcn_exp2f(t - mc);
}

template <typename T>
__global__ __launch_bounds__(BNT) void attn_bwd_kernel(const BwdParams bp) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub
  using V8 = typename MF<T>::v8;
  using V4 = typename MF<T>::v4;
  constexpr int CH = (KVB * 16) / BNT;  // 16-byte chunks of one K / V tile per thread (4)
  constexpr int ROWSTEP = BNT / 16;     // rows between a thread's consecutive chunks (16)
  const Params& p = bp.p;

  __shared__ __attribute__((aligned(16))) char smem[BWD_LDS];

  // ---- work decomposition ----
  const int wg = live_order(p, blockIdx.x, gridDim.x, p.xcd_remap);
  const int n_qb = p.n_groups * p.blocks_per_group;
  const int qb = wg % n_qb;
  const int y = wg / n_qb;
  if (p.n_heads_dev && y >= *p.n_heads_dev) return;
  const int head = p.head_list ? p.head_list[y] : y;
  int grp, p0, pend;
  if (p.q_block_table) {
    const int32_t* t = p.q_block_table + 3 * (qb / bp.sub);
    grp = t[0]; p0 = t[1] + (qb % bp.sub) * BQB; pend = t[2];
  } else {
    q_block_of(p, qb, BQB, grp, p0, pend);
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
    if (bp.do_scale) w = (float)((const T*)bp.do_scale)[(int64_t)head * bp.do_scale_sh];
    const char* qh = p.q + (int64_t)head * p.q_sh + lcc * 16;
    const char* gh = bp.d_o + (int64_t)head * bp.do_sh + lcc * 16;
    for (int i = 0; i < BQB / ROWSTEP; ++i) {
      const int row = lrow0 + i * ROWSTEP;
      const int pos = p0 + row;
      const bool ok = pos < pend && pos < q_valid;
      const int ldp = min(pos, pend - 1);
      const int64_t r = q_rows ? (int64_t)q_rows[ldp] : (int64_t)(p.q_row_offset + ldp);
      const int dst = tile_off(row, lcc * 8);
      *(u32x4*)(smem + Q_OFF + dst) = *(const u32x4*)(qh + r * p.q_ss);
      V8 g8;
      if (ok) {
        float acc[8];
        const V8 g0 = *(const V8*)(gh + r * bp.do_ss);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = (float)g0[e];
        if (p.dup_rows && pos < p.n_dup_pos) {
          const int32_t* dr = p.dup_rows + (int64_t)y * p.dup_rows_sh + (int64_t)pos * p.n_dup;
          for (int j = 0; j < p.n_dup; ++j) {
            const V8 gj = *(const V8*)(gh + (int64_t)dr[j] * bp.do_ss);
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
      *(V8*)(smem + DO_OFF + dst) = g8;
    }
  }
  __syncthreads();

  // ---- this lane's query: fragments of q and dO_eff (B operands of the score-shaped products) ----
  const int my_q = wave * 32 + r32;  // row of the block
  const int my_p = p0 + my_q;
  V8 qf[8], gf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    qf[ks] = *(const V8*)(smem + Q_OFF + tile_off(my_q, (2 * ks + hh) * 8));
    gf[ks] = *(const V8*)(smem + DO_OFF + tile_off(my_q, (2 * ks + hh) * 8));
  }

  // ---- K / V loader (global -> registers one block ahead -> LDS), as the forward's plain kernel ----
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
#define ISSUE_K() _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) kreg[i_] = *(const u32x4*)(kbase + nrow[i_] * p.k_ss);
#define ISSUE_V() _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) vreg[i_] = *(const u32x4*)(vbase + nrow[i_] * p.v_ss);
#define WRITE_K() _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) *(u32x4*)(smem + K_OFF + t_wr[i_]) = kreg[i_];
#define WRITE_V() _Pragma("unroll") for (int i_ = 0; i_ < CH; ++i_) *(u32x4*)(smem + V_OFF + t_wr[i_]) = vreg[i_];

  // fragment reads of a key tile as the A operand of a score-shaped product: key row r32 (+32), 8 channels
  int k_rd[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) k_rd[ks] = tile_off(r32, (2 * ks + hh) * 8);
  // (row + 32 keeps row & 15: the second half is the same offset + 32 rows)
#define SCORES(d0_, d1_, off_, b_)                                                \
  {                                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) { d0_[i_] = 0.f; d1_[i_] = 0.f; } \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 8; ++ks_) {                         \
      const V8 a0_ = *(const V8*)(smem + (off_) + k_rd[ks_]);                     \
      const V8 a1_ = *(const V8*)(smem + (off_) + k_rd[ks_] + 32 * ROWB);         \
      d0_ = MF<T>::mfma(a0_, b_[ks_], d0_);                                       \
      d1_ = MF<T>::mfma(a1_, b_[ks_], d1_);                                       \
    }                                                                             \
  }
#define MASK_TAIL(blk_, d0_, d1_)                                                 \
  if ((blk_) * KVB + KVB > n_kv) {                                                \
    _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) {                           \
      const int row_ = (i_ & 3) + 8 * (i_ >> 2) + 4 * hh;                         \
      if ((blk_) * KVB + row_ >= n_kv) d0_[i_] = -INFINITY;                       \
      if ((blk_) * KVB + 32 + row_ >= n_kv) d1_[i_] = -INFINITY;                  \
    }                                                                             \
  }

  const float c = p.scale_log2;

#define EXPO(s_, mc_) expo((s_), c, (mc_))

  // ---- pass 1: row maximum, row sum and delta ----
  float m_run = -1e30f, l_run = 0.f, d_run = 0.f;
  FETCH_ROWS(0);
  ISSUE_K();
  ISSUE_V();
  for (int blk = 0; blk < nblk; ++blk) {
    WRITE_K();
    WRITE_V();
    __syncthreads();
    if (blk + 1 < nblk) {
      FETCH_ROWS(blk + 1);
      ISSUE_K();
      ISSUE_V();
    }
    f32x16 s0, s1, g0, g1;
    SCORES(s0, s1, K_OFF, qf)
    SCORES(g0, g1, V_OFF, gf)
    MASK_TAIL(blk, s0, s1)
    float mx = s0[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s0[i]);
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s1[i]);
    mx = half_max(mx);
    const float m_new = fmaxf(m_run, mx);
    if (m_new != m_run) {
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
      l_run *= alpha;
      d_run *= alpha;
      m_run = m_new;
    }
    const float mc1 = rounded_mul(m_run, c);
    float lsum = 0.f, dsum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float e0 = EXPO(s0[i], mc1), e1 = EXPO(s1[i], mc1);
      lsum += e0 + e1;
      dsum += e0 * g0[i] + e1 * g1[i];
    }
    l_run += lsum;
    d_run += dsum;
    __syncthreads();
  }
  const float l_tot = half_sum(l_run);
  const float inv_l = l_tot > 0.f ? 1.f / l_tot : 0.f;
  const float mc = rounded_mul(m_run, c);
  const float delta = half_sum(d_run) * inv_l;

  // ---- pass 2 ----
  f32x16 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[dt][i] = 0.f;

  // transposed reads (ds_read_b64_tr_b16): a lane addresses row k0 + 4 hh + (lane & 15) / 4, elements n0 + 16 (lane / 16 & 1)
  // + 4 (lane & 3) of a row-major [k][n] image and receives, for n = n0 + r32, the four k = k0 + 4 hh + 0..3; two reads
  // (k0, k0 + 8) fill the eight k slots of a lane -- the same k order on both operands of every product below
  const int tr_row = 4 * hh + ((lane & 15) >> 2);
  const int tr_col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const int d0 = 32 * wave;  // phase B: this wave's channels

  FETCH_ROWS(0);
  ISSUE_K();
  ISSUE_V();
  WRITE_K();
  WRITE_V();
  if (1 < nblk) {
    FETCH_ROWS(1);
    ISSUE_K();
    ISSUE_V();
  }
  __syncthreads();

  for (int blk = 0; blk < nblk; ++blk) {
    // ================= phase A: this wave's 32 queries =================
    {
      f32x16 s0, s1, g0, g1;
      SCORES(s0, s1, K_OFF, qf)
      SCORES(g0, g1, V_OFF, gf)
      MASK_TAIL(blk, s0, s1)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s0[i] = EXPO(s0[i], mc) * inv_l;
        s1[i] = EXPO(s1[i], mc) * inv_l;
        g0[i] = s0[i] * (g0[i] - delta);
        g1[i] = s1[i] * (g1[i] - delta);
      }
      V8 dsb[4];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dsb[0][j] = (T)g0[j];
        dsb[1][j] = (T)g0[8 + j];
        dsb[2][j] = (T)g1[j];
        dsb[3][j] = (T)g1[8 + j];
      }
      // the [query][key] images: register group rg of a 32-key half holds keys 8 rg + 4 hh + 0..3 of this lane's query
      char* prow = smem + P_OFF + my_q * PSTRIDE + hh * 8;
      char* srow = smem + DS_OFF + my_q * PSTRIDE + hh * 8;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        V4 a, b, cc, d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = (T)s0[4 * rg + j];
          b[j] = (T)s1[4 * rg + j];
          cc[j] = dsb[rg >> 1][4 * (rg & 1) + j];
          d[j] = dsb[2 + (rg >> 1)][4 * (rg & 1) + j];
        }
        *(V4*)(prow + 16 * rg) = a;
        *(V4*)(prow + 64 + 16 * rg) = b;
        *(V4*)(srow + 16 * rg) = cc;
        *(V4*)(srow + 64 + 16 * rg) = d;
      }
      // dQ^T[d][q] += K^T . dS^T
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
          const V4 lo = MF<T>::tr(smem + K_OFF + tile_off(16 * kg + tr_row, 32 * dt + tr_col));
          const V4 hi = MF<T>::tr(smem + K_OFF + tile_off(16 * kg + 8 + tr_row, 32 * dt + tr_col));
          V8 kf;
#pragma unroll
          for (int j = 0; j < 4; ++j) { kf[j] = lo[j]; kf[4 + j] = hi[j]; }
          dq[dt] = MF<T>::mfma(kf, dsb[kg], dq[dt]);
        }
      }
    }
    __syncthreads();  // P / dS images complete; every wave is done with the K / V tiles
    if (blk + 1 < nblk) {
      WRITE_K();
      WRITE_V();
      if (blk + 2 < nblk) {
        FETCH_ROWS(blk + 2);
        ISSUE_K();
        ISSUE_V();
      }
    }
    // ================= phase B: dV, dK of this key block over all 128 queries =================
    {
      f32x16 av[2], ak[2];
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int i = 0; i < 16; ++i) { av[kh][i] = 0.f; ak[kh][i] = 0.f; }
#pragma unroll
      for (int kq = 0; kq < BQB / 16; ++kq) {
        const int qa = 16 * kq + tr_row, qc = qa + 8;
        V8 xg, xq;
        {
          const V4 lo = MF<T>::tr(smem + DO_OFF + tile_off(qa, d0 + tr_col));
          const V4 hi = MF<T>::tr(smem + DO_OFF + tile_off(qc, d0 + tr_col));
          const V4 lo2 = MF<T>::tr(smem + Q_OFF + tile_off(qa, d0 + tr_col));
          const V4 hi2 = MF<T>::tr(smem + Q_OFF + tile_off(qc, d0 + tr_col));
#pragma unroll
          for (int j = 0; j < 4; ++j) { xg[j] = lo[j]; xg[4 + j] = hi[j]; xq[j] = lo2[j]; xq[4 + j] = hi2[j]; }
        }
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
          const int col = (32 * kh + tr_col) * 2;
          const V4 lo = MF<T>::tr(smem + P_OFF + qa * PSTRIDE + col);
          const V4 hi = MF<T>::tr(smem + P_OFF + qc * PSTRIDE + col);
          const V4 lo2 = MF<T>::tr(smem + DS_OFF + qa * PSTRIDE + col);
          const V4 hi2 = MF<T>::tr(smem + DS_OFF + qc * PSTRIDE + col);
          V8 yp, ys;
#pragma unroll
          for (int j = 0; j < 4; ++j) { yp[j] = lo[j]; yp[4 + j] = hi[j]; ys[j] = lo2[j]; ys[4 + j] = hi2[j]; }
          av[kh] = MF<T>::mfma(yp, xg, av[kh]);  // [key][d]: rows = keys, this lane's column = channel d0 + r32
          ak[kh] = MF<T>::mfma(ys, xq, ak[kh]);
        }
      }
      float* dvh = bp.dv + (int64_t)head * bp.dv_sh + d0 + r32;
      float* dkh = bp.dk + (int64_t)head * bp.dk_sh + d0 + r32;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int pos = blk * KVB + 32 * kh + (i & 3) + 8 * (i >> 2) + 4 * hh;
          if (pos < n_kv) {
            const int64_t row = kv_rows ? (int64_t)kv_rows[pos] : (int64_t)(p.kv_row_offset + pos);
            unsafeAtomicAdd(dvh + row * bp.dv_ss, av[kh][i]);
            unsafeAtomicAdd(dkh + row * bp.dk_ss, ak[kh][i] * bp.scale);
          }
        }
      }
    }
    __syncthreads();  // the next K / V tiles are in place; the P / dS images are free
  }
#undef FETCH_ROWS
#undef ISSUE_K
#undef ISSUE_V
#undef WRITE_K
#undef WRITE_V
#undef SCORES
#undef MASK_TAIL
#undef EXPO

  // ---- epilogue: dq[r(p)] += scale dQ (one writer per row inside a launch) ----
  if (my_p >= pend || my_p >= q_valid) return;
  const int64_t my_row = q_rows ? (int64_t)q_rows[my_p] : (int64_t)(p.q_row_offset + my_p);
  float* dqp = bp.dq + (int64_t)head * bp.dq_sh + my_row * bp.dq_ss + 4 * hh;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      f32x4* dst = (f32x4*)(dqp + 32 * dt + 8 * rg);
      f32x4 v = *dst;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += dq[dt][4 * rg + j] * bp.scale;
      *dst = v;
    }
#endif
}

bool f32_ok(const vorta_tensor& t) {
  return t.ptr && !((uintptr_t)t.ptr & 15) && t.stride_s % 4 == 0 && t.stride_h % 4 == 0 && t.stride_s >= D;
}

}  // namespace

extern "C" int vorta_attn_bwd(const vorta_attn_bwd_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_attn_bwd_args)) return VORTA_EINVAL;
  // the forward's validation and geometry, for 128-row workgroups over the whole key list (split keys, the forward's
  // workspaces and its kernel variant change nothing in the gradient)
  vorta_attn_args f = a->fwd;
  f.n_splits = 1; f.ws_o = nullptr; f.ws_ml = nullptr;
  f.variant = 1;  // 64-bit K / V addressing: no window limit to check
  BwdParams bp{};
  int block_rows = 0;
  int rc = fill_params(&f, bp.p, block_rows, 2);
  if (rc != VORTA_OK) return rc;
  if (bp.p.n_heads == 0 || bp.p.n_groups == 0) return VORTA_OK;
  bp.sub = 1;
  if (f.q_block_table) {
    bp.sub = block_rows / BQB;  // a 256-row table row is two workgroups here
    bp.p.n_groups *= bp.sub;
  } else if (block_rows != BQB) {
    f.block_rows = BQB;
    rc = fill_params(&f, bp.p, block_rows, 2);
    if (rc != VORTA_OK) return rc;
  }
  Params& p = bp.p;
  p.n_splits = 1;
  p.wg_per_slot = p.n_groups * p.blocks_per_group;
  const vorta_tensor& g = a->d_o;
  if (!g.ptr || ((uintptr_t)g.ptr & 15) || (g.stride_s % 8) || (g.stride_h % 8) || g.stride_s < D) return VORTA_EINVAL;
  if (!f32_ok(a->dq) || !f32_ok(a->dk) || !f32_ok(a->dv)) return VORTA_EINVAL;
  bp.d_o = (const char*)g.ptr; bp.do_sh = g.stride_h * 2; bp.do_ss = g.stride_s * 2;
  bp.do_scale = a->do_scale; bp.do_scale_sh = a->do_scale_stride_h;
  bp.dq = (float*)a->dq.ptr; bp.dk = (float*)a->dk.ptr; bp.dv = (float*)a->dv.ptr;
  bp.dq_sh = a->dq.stride_h; bp.dq_ss = a->dq.stride_s;
  bp.dk_sh = a->dk.stride_h; bp.dk_ss = a->dk.stride_s;
  bp.dv_sh = a->dv.stride_h; bp.dv_ss = a->dv.stride_s;
  bp.scale = f.scale;
  const int64_t total = (int64_t)p.wg_per_slot * p.n_heads;
  if (total > 0x7fffffff) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  if (f.dtype == VORTA_BF16) hipLaunchKernelGGL(attn_bwd_kernel<__bf16>, dim3((unsigned)total), dim3(BNT), 0, st, bp);
  else hipLaunchKernelGGL(attn_bwd_kernel<_Float16>, dim3((unsigned)total), dim3(BNT), 0, st, bp);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
