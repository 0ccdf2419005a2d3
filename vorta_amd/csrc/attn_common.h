// Shared pieces of the gather flash-attention kernel families (attn_fwd.hip: 16 bits; attn_fwd_fp8.hip: all e4m3;
// attn_fwd_mx.hip: 16-bit scores, e4m3 P V; attn_fwd_i8.hip: int8 scores, e4m3 P V): the launch parameters, the fused-grid
// block, the split-key merge, the host launch path, and the two ends of a kernel body -- decode_work (logical workgroup ->
// what it works on) and write_rows (the epilogue).
// ONLY attn_i8_body calls the two ends so far.  The other four bodies (attn_fwd_kernel, attn_pipe_dma_body, attn8_body,
// attn_mx_body) still carry their own copies of both, so a change to the decode or the epilogue has to be made in FIVE places:
// here and in each of them.  All four were built on these functions and put back: attn_fwd_kernel and attn8_body parked more
// SGPRs in VGPR lanes than before (attn8 also inside its key loop), attn_pipe_dma_body measured 0.4 % slower on the fused
// layer kernel, attn_mx_body spilled VGPRs (profiles/attn_fwd_shared_pieces_resources.txt, _timing.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace vorta_attn {


constexpr int KVB = 64;            // keys per block
constexpr int D = 128;             // head dim
constexpr int ROWB = D * 2;        // bytes per row
constexpr int TILE_BYTES = KVB * ROWB;  // 16 KiB
constexpr int BUF_BYTES = 2 * TILE_BYTES;

struct Params {
  const char* q; const char* k; const char* v; char* o;
  int64_t q_sh, k_sh, v_sh, o_sh;  // head strides in bytes
  int64_t q_ss, k_ss, v_ss, o_ss;  // row strides in bytes
  const int32_t* head_list; const int32_t* n_heads_dev;
  int n_heads;
  int n_q, q_group_len, q_row_offset, q_valid;
  int n_groups, blocks_per_group;
  const int32_t* q_rows; int64_t q_rows_sh;
  int n_kv, kv_row_offset;
  const int32_t* n_kv_dev; const int32_t* q_valid_dev;
  const int32_t* kv_rows; int64_t kv_rows_sh, kv_rows_sg;
  const int32_t* dup_rows; int64_t dup_rows_sh; int n_dup_pos, n_dup;
  float scale_log2;  // scale * log2(e)
  int n_splits, blocks_per_split;
  float* ws_o; float* ws_ml;
  int xcd_remap;
  float defer_log2;  // online-softmax rescale is skipped while the row max grows by <= this (log2 units)
  const int32_t* q_block_table;  // optional [n_groups * blocks_per_group][3] = (group, first position, end position)
  int wg_per_slot;               // workgroups of one head slot = n_groups * blocks_per_group * n_splits
};

// query block qb of a launch -> its group (key list), first position and the end of its positions
__device__ __forceinline__ void q_block_of(const Params& p, int qb, int rows_per_block, int& grp, int& p0, int& pend) {
  if (p.q_block_table) {
    const int32_t* t = p.q_block_table + 3 * qb;
    grp = t[0]; p0 = t[1]; pend = t[2];
  } else {
    grp = qb / p.blocks_per_group;
    p0 = grp * p.q_group_len + (qb - grp * p.blocks_per_group) * rows_per_block;
    pend = min((grp + 1) * p.q_group_len, p.n_q);
  }
}

// Logical workgroup id of physical block b of a launch (or of a fused segment) with n ids.
// XCD-aware order: workgroups whose ids are equal mod 8 share an XCD (round-robin dispatch), so each such class gets a
// contiguous chunk of the logical ids (same head, neighbouring query blocks: one L2 serves the K/V stream instead of
// eight).  With a device-resident head count (n_heads_dev) the grid is sized for every head slot but only the first
// *n_heads_dev are live: the chunks are cut from the LIVE ids, so all eight XCDs share the live work to within one
// workgroup; a dead block keeps its own id, which decodes to a slot >= *n_heads_dev, and leaves through the body's slot
// check (no second exit path: one in the kernel wrappers cost the single-launch e4m3 kernels 36-100 B of scratch).  (Cut from all n ids -- slot-major -- the live third of a uniform
// Hunyuan layer landed on three XCDs: the device-routed fused launch took 201 ms against 68 ms with host counts;
// spreading whole slots instead left 14 live slots of 40 at 2 + 2 + ... + 1 + 1 per XCD, 13 % over the host-count time.)
__device__ __forceinline__ int live_order(const Params& p, int b, int n, bool remap) {
  if (p.n_heads_dev) n = min(n, max(*p.n_heads_dev, 0) * p.wg_per_slot);
  if (!remap || b >= n) return b;
  const int xcd = b & 7, qd = n >> 3, r = n & 7;
  return (xcd < r ? xcd * (qd + 1) : r * (qd + 1) + (xcd - r) * qd) + (b >> 3);
}

// What logical workgroup wg of a launch works on: split sp of the key blocks [blk0, blk1) of head slot y (tensor head
// `head`), for the query positions [p0, pend) of group grp (its key list); n_kv and q_valid with their device-resident
// values applied (no host sync)
struct Work {
  int sp, y, head, grp, p0, pend, n_kv, q_valid, blk0, blk1;
};

// Fills w for a workgroup of QB query rows.  False: a dead head slot (y >= *n_heads_dev, see live_order) -- the body returns.
template <int QB>
__device__ __forceinline__ bool decode_work(const Params& p, int wg, Work& w) {
  w.sp = wg % p.n_splits;
  const int rest = wg / p.n_splits;
  const int n_qb = p.n_groups * p.blocks_per_group;
  w.y = rest / n_qb;
  if (p.n_heads_dev && w.y >= *p.n_heads_dev) return false;
  // (UNI: what this workgroup reads from device memory through a workgroup-uniform address stays in scalar registers.  The
  // compiler proves that by itself only in a kernel that writes no memory in front of the load; the fused kernel's ticket
  // draw does, and without this the query block's bounds became vector values that lived across the loops: 2 spilled VGPRs)
#define UNI(x_) __builtin_amdgcn_readfirstlane(x_)
  w.head = p.head_list ? UNI(p.head_list[w.y]) : w.y;
  q_block_of(p, rest % n_qb, QB, w.grp, w.p0, w.pend);
  w.grp = UNI(w.grp); w.p0 = UNI(w.p0); w.pend = UNI(w.pend);
  w.n_kv = p.n_kv_dev ? max(1, min(UNI(*p.n_kv_dev), p.n_kv)) : p.n_kv;
  w.q_valid = p.q_valid_dev ? min(UNI(*p.q_valid_dev), p.q_valid) : p.q_valid;
#undef UNI
  w.blk0 = w.sp * p.blocks_per_split;
  w.blk1 = min(w.blk0 + p.blocks_per_split, (w.n_kv + KVB - 1) / KVB);
  return true;
}

// Tensor row of query position pos of w (a position past the end of the query block repeats the block's last row)
__device__ __forceinline__ int64_t q_row_of(const Params& p, const Work& w, int pos) {
  pos = min(pos, w.pend - 1);
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)w.y * p.q_rows_sh : nullptr;
  return q_rows ? (int64_t)q_rows[pos] : (int64_t)(p.q_row_offset + pos);
}

#ifndef VORTA_MAX_SEGMENTS
#define VORTA_MAX_SEGMENTS VORTA_MAX_FUSED_LAUNCHES /* include/vorta_hip.h */
#endif
constexpr int MAX_SEGMENTS = VORTA_MAX_SEGMENTS;  // launches fused into one grid (vorta_attn_fwd_batch): three experts, the text queries or up to
                                 // two partial full-attention heads of a sequence-parallel rank (ulysses/engine.py split_placement)
// Params8, ParamsMx and ParamsI8 extend a Params `p` with their family's fields; base_of reaches the common part of any block
template <class PP> __host__ __device__ __forceinline__ Params& base_of(PP& pp) { return pp.p; }
template <class PP> __host__ __device__ __forceinline__ const Params& base_of(const PP& pp) { return pp.p; }
__host__ __device__ __forceinline__ Params& base_of(Params& p) { return p; }
__host__ __device__ __forceinline__ const Params& base_of(const Params& p) { return p; }

template <class PP> struct MultiOf {
  PP seg[MAX_SEGMENTS];
  int start[MAX_SEGMENTS + 1];  // first workgroup of each segment; start[n] = grid size
  int n;
};

// Segment of physical block b of a fused grid, and (wg) its logical workgroup id in XCD-aware order INSIDE the segment:
// workgroups whose ids are equal mod 8 share an XCD (round-robin dispatch), so each such class gets a contiguous chunk of
// the segment's logical ids (same head, neighbouring query blocks -> one L2 serves the K/V stream instead of eight).  Every
// XCD still gets 1/8 of every segment, which keeps the chip balanced across segments of different cost.
template <class PP>
__device__ __forceinline__ int segment_index(const MultiOf<PP>& mp, int b, int& wg) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < MAX_SEGMENTS; ++i) s += (i < mp.n && b >= mp.start[i]) ? 1 : 0;
  wg = live_order(base_of(mp.seg[s]), b - mp.start[s], mp.start[s + 1] - mp.start[s], true);
  return s;
}
template <class PP>
__device__ __forceinline__ const PP& segment_of(const MultiOf<PP>& mp, int b, int& wg) {
  return mp.seg[segment_index(mp, b, wg)];
}

// Ticket order of a fused grid (the 16-bit family; vorta_attn_fwd_batch_tickets).  cnt[s * 8 + x] counts the tickets drawn
// from the share of XCD class x (= block index & 7) in segment s: the chunk of the segment's live logical ids that
// live_order gives that class, drawn in the same order.  A workgroup draws from its own class, segments in order; when
// its class has nothing left in any segment it draws from the (segment, class) with the most left.  It returns the
// segment (wg = the logical workgroup there), or -1 when every counter is exhausted -- the grid has at least one block per
// live or dead logical id (grid_blocks below) and a block exits only when nothing is left, so every live id is drawn.
// No workgroup waits for another: a draw that loses a race sees that counter exhausted on its next read (counters only
// grow), so the loop ends after at most one round per counter.  The counters are read and advanced at agent scope: the
// XCDs' L2s are not coherent with each other.  Called by all 64 lanes of one wave; TICKET_INTS counters, zero at launch.
constexpr int TICKET_INTS = 8 * MAX_SEGMENTS + 8;  // (the last eight are spare: the size the header promises)
static_assert(MAX_SEGMENTS <= 8, "draw_ticket keeps one (segment, class) pair per lane");
template <class PP>
__device__ __forceinline__ int draw_ticket(const MultiOf<PP>& mp, int32_t* cnt, int b, int& wg) {
  const int lane = threadIdx.x & 63;
  const int x_l = lane & 7;
  int len_l = 0, base_l = 0;  // lane s * 8 + x: the share of class x in segment s
#pragma unroll
  for (int i = 0; i < MAX_SEGMENTS; ++i) {
    if (i < mp.n) {
      const Params& p = base_of(mp.seg[i]);
      int n = mp.start[i + 1] - mp.start[i];
      if (p.n_heads_dev) n = min(n, max(*p.n_heads_dev, 0) * p.wg_per_slot);
      const int qd = n >> 3, r = n & 7;
      if ((lane >> 3) == i) {
        len_l = qd + (x_l < r ? 1 : 0);
        base_l = x_l < r ? x_l * (qd + 1) : r * (qd + 1) + (x_l - r) * qd;
      }
    }
  }
  for (;;) {
    int left = 0;
    if (len_l > 0) left = max(len_l - __hip_atomic_load(cnt + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0);
    int pick;
    const unsigned long long own = __ballot(left > 0 && x_l == (b & 7));
    if (own) {
      pick = __ffsll(own) - 1;
    } else {
      int most = left;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
      if (most == 0) return -1;
      pick = __ffsll(__ballot(left == most)) - 1;
    }
    int t = 0;
    if (lane == pick) t = __hip_atomic_fetch_add(cnt + lane, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = __shfl(t, pick);
    if (t < __shfl(len_l, pick)) {
      wg = __shfl(base_l, pick) + t;
      return pick >> 3;
    }
  }
}

// Per-channel factor of the merged output: v_descale[head] for the families with e4m3 V, none in 16 bits
__device__ __forceinline__ float2 out_descale(const Params&, int, int) { return make_float2(1.f, 1.f); }
template <class PP> __device__ __forceinline__ float2 out_descale(const PP& pp, int head, int lane) {
  return *(const float2*)(pp.v_descale + (int64_t)head * pp.v_descale_sh + lane * 2);
}
// The same for a single-pass epilogue, folded into the row's 1/l: what multiplies the accumulators of the four channels
// from ch on (16 bits: inv alone -- no load, no multiply by 1)
__device__ __forceinline__ f32x4 out_descale4(const Params&, int, int, float inv) { return f32x4{inv, inv, inv, inv}; }
template <class PP> __device__ __forceinline__ f32x4 out_descale4(const PP& pp, int head, int ch, float inv) {
  const f32x4 s = *(const f32x4*)(pp.v_descale + (int64_t)head * pp.v_descale_sh + ch);
  return f32x4{inv * s[0], inv * s[1], inv * s[2], inv * s[3]};
}

// Merge the split-key partials: one wave per (head slot, query position).  The partials are unnormalised (in the e4m3-P
// families both sums carry the 2^p_bias factor) and the reference points are in the exp2 domain.
template <typename T, class PP>
__global__ __launch_bounds__(256) void attn_combine_kernel(const PP pp) {
  const Params& p = base_of(pp);
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (int64_t)p.n_heads * p.n_q) return;
  const int y = (int)(item / p.n_q);
  const int pos = (int)(item - (int64_t)y * p.n_q);
  if (p.n_heads_dev && y >= *p.n_heads_dev) return;
  const int head = p.head_list ? p.head_list[y] : y;
  float m = -1e30f;
  for (int s = 0; s < p.n_splits; ++s) m = fmaxf(m, p.ws_ml[(((int64_t)y * p.n_splits + s) * p.n_q + pos) * 2]);
  float acc0 = 0.f, acc1 = 0.f, l = 0.f;
  for (int s = 0; s < p.n_splits; ++s) {
    const int64_t slot = ((int64_t)y * p.n_splits + s) * p.n_q + pos;
    const float w = __builtin_amdgcn_exp2f(p.ws_ml[slot * 2] - m);
    l += w * p.ws_ml[slot * 2 + 1];
    const float2 v = *(const float2*)(p.ws_o + slot * D + lane * 2);
    acc0 += w * v.x;
    acc1 += w * v.y;
  }
  const int q_valid = p.q_valid_dev ? min(*p.q_valid_dev, p.q_valid) : p.q_valid;
  // a position past q_valid is written as zero bits whatever its partials hold (0 x NaN is NaN, 0 x a negative sum is
  // -0): a select on the position alone, applied to the converted values.  A position below q_valid keeps its
  // arithmetic: a NaN row sum still gives a NaN row
  const bool past = pos >= q_valid;
  const float inv = (!past && l > 0.f) ? 1.f / l : 0.f;
  const float2 sd = out_descale(pp, head, lane);
  const int32_t* q_rows = p.q_rows ? p.q_rows + (int64_t)y * p.q_rows_sh : nullptr;
  const int64_t row = q_rows ? (int64_t)q_rows[pos] : (int64_t)(p.q_row_offset + pos);
  const T pair[2] = {(T)(acc0 * inv * sd.x), (T)(acc1 * inv * sd.y)};
  // The two converted values are ONE opaque register from here on, stored to the row and to its duplicates.  Written
  // as two reads of `pair`, the fp16 instantiation gave a duplicate row that differed from its source row by one ulp in
  // about one element of ten thousand, each next to a rounding midpoint (tests/test_hip_attention_fwd_structured.py,
  // the gather launches with splits).  The cause was not established; presumably the conversion was emitted once per
  // store, fused with the multiply (one rounding) in one place and after it (two roundings) in the other.
  uint32_t bits;
  __builtin_memcpy(&bits, pair, sizeof(bits));
  if (past) bits = 0u;
  asm volatile("" : "+v"(bits));
  char* ob = p.o + (int64_t)head * p.o_sh + lane * 4;
  *(uint32_t*)(ob + row * p.o_ss) = bits;
  if (p.dup_rows && pos < p.n_dup_pos) {
    const int32_t* dr = p.dup_rows + (int64_t)y * p.dup_rows_sh + (int64_t)pos * p.n_dup;
    for (int i = 0; i < p.n_dup; ++i) *(uint32_t*)(ob + (int64_t)dr[i] * p.o_ss) = bits;
  }
}

// ---- host: the launch path of every family ----
// A family (one per source file) supplies only what differs:
//   F::PP                            its parameter block (Params, or one that extends it)
//   f.fill(a, pp, block_rows)        validation + launch geometry of one launch (the args and the family's ext)
//   f.fusable(a, pp)                 whether a 256-row launch may join a fused grid
//   f.out_dtype(a)                   VORTA_BF16 / VORTA_FP16: the output type T of the kernels
//   F::kernel<T>(a, pp, block_rows)  the single-launch kernel (block_rows / 32 waves)
//   F::multi<T>                      the fused-grid kernel (8 waves)

template <typename T, class PP>
int launch_combine(const PP& pp, hipStream_t st) {
  const Params& p = base_of(pp);
  if (p.n_splits <= 1) return VORTA_OK;
  const int64_t items = (int64_t)p.n_heads * p.n_q;
  hipLaunchKernelGGL((attn_combine_kernel<T, PP>), dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, pp);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

template <typename T, class PP>
int launch_single(void (*kernel)(PP), int block_rows, const PP& pp, hipStream_t st) {
  const Params& p = base_of(pp);
  const int64_t total = (int64_t)p.n_groups * p.blocks_per_group * p.n_heads * p.n_splits;
  if (total <= 0) return VORTA_OK;
  if (total > 0x7fffffff) return VORTA_EINVAL;
  hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(block_rows * 2), 0, st, pp);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vorta_set_hip_error(e);
  return launch_combine<T>(pp, st);
}

// vorta_attn_fwd and its siblings: one launch of the family's kernel, then the split-key merge
template <class F>
int fwd_single(const F& f, const vorta_attn_args* a, void* hip_stream) {
  typename F::PP pp{};
  int block_rows = 0;
  const int rc = f.fill(a, pp, block_rows);
  if (rc != VORTA_OK) return rc;
  if (base_of(pp).n_heads == 0 || base_of(pp).n_groups == 0) return VORTA_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  if (f.out_dtype(*a) == VORTA_BF16) return launch_single<__bf16>(F::template kernel<__bf16>(*a, pp, block_rows), block_rows, pp, st);
  return launch_single<_Float16>(F::template kernel<_Float16>(*a, pp, block_rows), block_rows, pp, st);
}

// What a fused grid needs enqueued in front of it, by the further arguments of the family's fused kernel: nothing, or (the
// 16-bit family's ticket counters) their reset.  A one-block kernel on the launch stream rather than a reset by the grid's
// last workgroup: it is a node of a captured graph like the grid itself, so every replay starts from zero as well, it costs
// the grid no counter of arrivals and no agent-scope release, and a launch that was cut short cannot leave the counters
// of the next one dirty.  (Not hipMemsetAsync: captured with the layer in a torch.cuda.graph, the counters were zero for
// the first replay only and the second replay's workgroups found them exhausted -- tests/test_hip_fused_ticket_order.py.)
template <int N>
__global__ void ticket_reset_kernel(int32_t* cnt) {
  if (threadIdx.x < N) cnt[threadIdx.x] = 0;
}
inline int before_grid(hipStream_t) { return VORTA_OK; }
template <class I>  // (a template, so that only the object that passes counters holds the reset kernel)
int before_grid(hipStream_t st, I* tickets) {
  if (!tickets) return VORTA_OK;
  hipLaunchKernelGGL(ticket_reset_kernel<TICKET_INTS>, dim3(1), dim3(64), 0, st, tickets);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

// Blocks of a fused grid with `total` logical workgroups.  In ticket order an eighth more (a multiple of 8, so every XCD
// class gets the same): the hardware deals blocks to the XCDs round-robin whatever their load, so with one block per
// ticket every XCD runs exactly its eighth of the blocks however early it is done -- a traced Hunyuan layer in ticket
// order ended with the same 1 179 workgroups on every XCD, up to 5 ms apart (profiles/fused_grid_ticket_order.txt).  The
// spare blocks are the last of their class to be dispatched: on an XCD that is done early they draw what the late ones
// have left, on the others they find every counter exhausted and exit.
inline int grid_blocks(int64_t total) { return (int)total; }
template <class I>
int grid_blocks(int64_t total, I* tickets) {
  if (!tickets) return (int)total;
  return (int)min((int64_t)0x7fffffff, total + ((total / 8 + 7) & ~(int64_t)7));
}

// (extra...: further kernel arguments of a family's fused kernel -- the 16-bit one takes its ticket counters)
template <typename T, class PP, class... X>
int launch_fused(void (*kernel)(MultiOf<PP>, X...), const MultiOf<PP>& mp, int total, hipStream_t st, X... extra) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(512), 0, st, mp, extra...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vorta_set_hip_error(e);
  for (int i = 0; i < mp.n; ++i) {
    const int rc = launch_combine<T>(mp.seg[i], st);
    if (rc != VORTA_OK) return rc;
  }
  return VORTA_OK;
}

// vorta_attn_fwd_batch and its siblings: up to MAX_SEGMENTS launches as the segments of ONE grid, in the given order.
// Empty launches are skipped; the others must resolve to the 256-row pipelined kernel and share one output type.
template <class F, class... X>
int fwd_batch(const F& f, const vorta_attn_args* args, int32_t n, void* hip_stream, X... extra) {
  if (!args || n < 0 || n > MAX_SEGMENTS) return VORTA_EINVAL;
  MultiOf<typename F::PP> mp{};
  int64_t total = 0;
  int dtype = -1, m = 0;
  for (int i = 0; i < n; ++i) {
    typename F::PP pp{};
    int block_rows = 0;
    const int rc = f.fill(&args[i], pp, block_rows);
    if (rc != VORTA_OK) return rc;
    Params& p = base_of(pp);
    if (p.n_heads == 0 || p.n_groups == 0) continue;
    if (block_rows != 256 || !f.fusable(args[i], pp)) return VORTA_EUNSUPPORTED;
    if (dtype >= 0 && dtype != f.out_dtype(args[i])) return VORTA_EINVAL;
    dtype = f.out_dtype(args[i]);
    p.xcd_remap = 0;  // segment_of orders the workgroups
    mp.seg[m] = pp;
    mp.start[m] = (int)total;
    total += (int64_t)p.n_groups * p.blocks_per_group * p.n_heads * p.n_splits;
    if (total > 0x7fffffff) return VORTA_EINVAL;
    ++m;
  }
  if (m == 0) return VORTA_OK;
  for (int i = m; i <= MAX_SEGMENTS; ++i) mp.start[i] = (int)total;
  mp.n = m;
  hipStream_t st = (hipStream_t)hip_stream;
  const int rc = before_grid(st, extra...);
  if (rc != VORTA_OK) return rc;
  const int blocks = grid_blocks(total, extra...);
  if (dtype == VORTA_BF16) return launch_fused<__bf16>(F::template multi<__bf16>, mp, blocks, st, extra...);
  return launch_fused<_Float16>(F::template multi<_Float16>, mp, blocks, st, extra...);
}

// attn_fwd.hip: argument validation + launch geometry (in_esize = bytes per q/k element, v_esize per v element: 0 = the
// same; args->dtype names the 2-byte type, or e4m3 when in_esize = 1)
// (k_esize: bytes per k element when it differs from q's -- the int8-score kernel reads 16-bit q and int8 k; 0 = the same)
int fill_params(const vorta_attn_args* a, Params& p, int& block_rows, int in_esize, int v_esize = 0, int k_esize = 0);
// attn_fwd_mx.hip: 16-bit scores, e4m3 P V (vorta_attn_fwd_fp8 / _batch_fp8 with ext->flags bit1)
int mx_fwd(const vorta_attn_args* a, const vorta_attn_fp8_ext* ext, void* hip_stream);
int mx_fwd_batch(const vorta_attn_args* args, const vorta_attn_fp8_ext* ext, int32_t n, void* hip_stream);

template <typename T> struct MF;
template <> struct MF<__bf16> {
  using v8 = bf16x8; using v4 = bf16x4;
  static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ v4 tr(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS v4*)p);
  }
};
template <> struct MF<_Float16> {
  using v8 = f16x8; using v4 = f16x4;
  static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ v4 tr(const char* p) {
    typedef __attribute__((ext_vector_type(4))) __fp16 h4;
    h4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((LDS_AS h4*)p);
    return *(v4*)&r;
  }
};

// v_permlane32_swap(vdst, src) exchanges lanes 32-63 of vdst with lanes 0-31 of src.  Fed the same value
// twice it returns {low half, low half} and {high half, high half}: combining the two results gives every
// lane the reduction over itself and its partner lane ^ 32 (the two lanes that share one query row).
__device__ __forceinline__ float half_max(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// The end of every forward body, for an active wave (first position wrow0): o = its unnormalised O^T accumulators (channel
// 32 dt + 8 (i / 4) + 4 hh + (i & 3) of the lane's row in o[dt][i]), m_ref = the row's reference point in the exp2 domain,
// l_tot = its row sum.  With key splits the partials go to ws_o / ws_ml for attn_combine_kernel; else the rows are
// normalised, converted to T and stored.
template <typename T, class PP>
__device__ __forceinline__ void write_rows(const PP& pp, const Work& w, int wrow0, const f32x16 (&o)[4], float m_ref, float l_tot) {
  const Params& p = base_of(pp);
  // The row bookkeeping (hh, pos and row: the body's hh, its lane's position and q_row_of) is derived again from the thread id,
  // opaque to the compiler, so that it is not the prologue's values kept in registers across both loops.  The 0 VGPR
  // spills / 0 scratch of vorta_amd.build.kernel_resources depend on it: with the prologue's values used here the
  // allocator spills them in front of the loops -- attn_fwd_multi_kernel 8 VGPRs (28 B of scratch), attn_fwd_pipe_kernel
  // <T, 8, true> 5 (24 B), <T, 8, false> 1 (8 B) -- and tests/test_build_resources.py fails.
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int hh = (tid >> 5) & 1;
  const int pos = wrow0 + (tid & 31);
  const bool ok = pos < w.pend;
  const int64_t row = q_row_of(p, w, pos);
  if (p.n_splits > 1) {
    // unnormalised partials (in the e4m3-P families both carry the 2^p_bias factor): ws_o[y][sp][pos][d], ws_ml[y][sp][pos][2]
    if (ok) {
      const int64_t slot = ((int64_t)w.y * p.n_splits + w.sp) * p.n_q + pos;
      float* wo = p.ws_o + slot * D;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          f32x4 v = {o[dt][4 * rg], o[dt][4 * rg + 1], o[dt][4 * rg + 2], o[dt][4 * rg + 3]};
          *(f32x4*)(wo + 32 * dt + 8 * rg + 4 * hh) = v;
        }
      if (hh == 0) {
        p.ws_ml[slot * 2] = m_ref;
        p.ws_ml[slot * 2 + 1] = l_tot;
      }
    }
    return;
  }
  if (!ok) return;
  // a position past q_valid is written as zero bits whatever its accumulators hold (0 x NaN is NaN, 0 x a negative sum
  // is -0): a select on the position alone, applied to the converted values.  A position below q_valid keeps its
  // arithmetic: a NaN row sum still gives a NaN row
  const bool past = pos >= w.q_valid;
  const float inv = (!past && l_tot > 0.f) ? 1.f / l_tot : 0.f;
  uint2 packed[16];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const f32x4 s = out_descale4(pp, w.head, 32 * dt + 8 * rg + 4 * hh, inv);
      typename MF<T>::v4 t;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = (T)(o[dt][4 * rg + j] * s[j]);
      packed[dt * 4 + rg] = past ? make_uint2(0u, 0u) : *(uint2*)&t;
    }
  char* obase = p.o + (int64_t)w.head * p.o_sh + hh * 8;
  // (a row and its duplicates are stores of the same `packed` values, converted once above.  No barrier as in
  // attn_combine_kernel pins that here: tried, it changed nothing that a test or the benchmark's outputs could show.
  // tests/test_hip_attention_fwd_structured.py compares every duplicate row with its source row as bits on each
  // gather launch, which is what holds the property)
  auto store_row = [&](int64_t r) {
    char* op = obase + r * p.o_ss;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) *(uint2*)(op + (32 * dt + 8 * rg) * 2) = packed[dt * 4 + rg];
  };
  store_row(row);
  if (p.dup_rows && pos < p.n_dup_pos) {
    const int32_t* dr = p.dup_rows + (int64_t)w.y * p.dup_rows_sh + (int64_t)pos * p.n_dup;
    for (int i = 0; i < p.n_dup; ++i) store_row((int64_t)dr[i]);
  }
}


}  // namespace vorta_attn
