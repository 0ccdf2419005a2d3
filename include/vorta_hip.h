/*
 * vorta_hip.h -- C ABI of libvorta_hip.so: the MI355X (gfx950) implementation of VORTA's routed
 * sparse-attention denoising hot path.
 *
 * The reference (wenhao728/VORTA) is pure Python and has no FFI of its own: the boundary it exposes is
 * the diffusers attention-processor protocol (vorta/attention/__init__.py:1-16).  Each entry point below
 * names the reference code it replaces (paths relative to the reference root).  The Python host side
 * (vorta_amd/) binds these with ctypes and mirrors the reference's processor classes one to one; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (VORTA_OK) or a negative VORTA_E* code; nothing throws across the ABI;
 *   - the caller owns every buffer (inputs, outputs, index tables, workspaces); the library allocates
 *     nothing and keeps no state; all pointers are DEVICE pointers unless a field says "host";
 *   - work is enqueued on the given hipStream_t (passed as void*); no call synchronises the device;
 *   - a "head slot" y in [0,n_heads) addresses head  head_list ? head_list[y] : y  of the (H,S,D) tensors;
 *     a batch is folded into the head axis by the caller (head = b*H + h with stride_h the same);
 *   - rows of D contiguous elements; strides in ELEMENTS; 16-byte aligned rows.
 */
#ifndef VORTA_HIP_H
#define VORTA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VORTA_OK 0
#define VORTA_EINVAL (-1)       /* bad argument (null pointer, size, alignment, struct_size)          */
#define VORTA_EUNSUPPORTED (-2) /* valid request this build does not implement (head_dim, dtype)      */
#define VORTA_ELAUNCH (-3)      /* the HIP runtime refused the launch (see vorta_last_hip_error)      */

#define VORTA_ABI_VERSION 9 /* 2: adds the fp8 entry points (vorta_fp8_*, vorta_attn_fwd_fp8*); 3: adds vorta_permute_heads;
                                4: vorta_fp8_quant_args gains slot_first / slot_count and flags bit2, adds vorta_fp8_v_absmax /
                                vorta_fp8_v_convert; every earlier call means what it meant
                                5: vorta_fp8_quant_args gains video_tokens / token_offset / total_tokens / src_map and flags
                                bit3 / bit4 (sequence shards), adds vorta_fp8_quant_ws_partials
                                6: adds the int8-score entry points (vorta_i8_quantize_k, vorta_attn_fwd_i8, vorta_attn_fwd_batch_i8);
                                7: the int8-score kernel writes its probabilities with one power-of-two scale per query row
                                   and 32 keys (vorta_attn_i8_ext.defer becomes the reference-point trigger in binades, default 24);
                                8: adds vorta_i8_tail_flags and vorta_split_heads (per-head choice between int8 and 16-bit scores)
                                9: adds the backward entry points (vorta_attn_bwd, vorta_mix_experts_bwd, vorta_cast_grads);
                                   9 also carries vorta_qk_norm_rope_bwd (a pure addition: every earlier call means what it meant;
                                   a binding asks for the symbol and for vorta_sizeof(16) to tell the two libraries apart)
                                   and the key-major backward, vorta_attn_bwd_stats / vorta_attn_bwd_kmajor (a pure addition too:
                                   a binding asks for the symbols and for vorta_attn_bwd_kmajor_args_size())
                                   and the deterministic backward, vorta_attn_bwd_dq / vorta_attn_bwd_dkv (two more symbols, on
                                   the key-major argument block)
                                   and the per-head expert fidelity, vorta_expert_fidelity (a pure addition: a binding asks for
                                   the symbol and for vorta_fidelity_args_size())
                                   and partial geometry, vorta_sta_partial_sizes / vorta_sta_build_tables_partial /
                                   vorta_coreset_select_partial (three more symbols on the existing argument blocks)
                                   and the routed output's fidelity on sampled rows, vorta_sampled_fidelity (a pure addition: a
                                   binding asks for the symbol and for vorta_sampled_fidelity_args_size())
                                   and the sampled rows of a per-expert measurement, vorta_gather_sample_rows (a pure addition:
                                   a binding asks for the symbol and for vorta_gather_sample_rows_args_size())
                                   and the fused 16-bit grid in ticket order, vorta_attn_fwd_batch_tickets /
                                   vorta_attn_ticket_workspace_ints (a pure addition: two more symbols on the existing
                                   argument block; an older ABI-9 library lacks them, which a binding sees at symbol lookup)
                                   and head routing from measured statistics, vorta_route_fidelity (a pure addition: a binding
                                   asks for the symbol and for vorta_route_fidelity_args_size())
                                   and the same over (precision tier, expert) pairs, vorta_route_fidelity_tiers (a pure
                                   addition: the symbol and vorta_route_fidelity_tiers_args_size())
                                   and the verification and repair of launched routes, vorta_route_repair (a pure addition:
                                   the symbol and vorta_route_repair_args_size())
                                   and routing over (precision tier, expert) pairs by a cost budget, vorta_route_budget_tiers (a
                                   pure addition: the symbol and vorta_route_budget_tiers_args_size()) */

typedef enum vorta_dtype {
  VORTA_BF16 = 0,
  VORTA_FP16 = 1,
  VORTA_FP32 = 2,    /* vorta_route_scores only */
  VORTA_FP8E4M3 = 3, /* OCP e4m3fn bytes: q/k/v of vorta_attn_fwd_fp8, output of vorta_fp8_quantize_qkv */
  VORTA_INT8 = 4     /* two's-complement bytes: k8 of vorta_i8_quantize_k / vorta_attn_fwd_i8 (vorta_permute_heads: any 1-byte rows) */
} vorta_dtype;

/* One (H,S,D) operand: element (h,s,d) lives at ptr + h*stride_h + s*stride_s + d. */
typedef struct vorta_tensor {
  void* ptr;
  int64_t stride_h;
  int64_t stride_s;
} vorta_tensor;

/*
 * vorta_attn_fwd -- softmax(Q K^T * scale) V for a list of heads, with row indirection.
 *
 * One generic gather flash-attention kernel serves all three experts:
 *   dense   (hunyuan.py:136-189 `_step_attention`, wan.py:103-149 `_attn`): no tables, n_kv = valid
 *           keys (Hunyuan L = attention_mask.sum(), hunyuan.py:169), q_valid = L so padded text rows
 *           come out exactly zero (hunyuan.py:176);
 *   coreset (hunyuan.py:410-457, wan.py:243-270 + coreset_select.py:68-185): q_rows / kv_rows are the
 *           keep-lists written by vorta_coreset_select, dup_rows its drop-lists: pool-gather and
 *           unpool-scatter are fused into the loads and the epilogue, no pooled copy exists;
 *   sliding tile (sliding_attn_flex.py:72-211 + tile.py:7-78): q_rows is the tile-major permutation,
 *           kv_rows the per-q-tile key list from vorta_sta_build_tables (q_group_len = tokens/tile);
 *           tile/untile are address arithmetic, no BlockMask and no permuted copy exists.
 * Each head writes straight into its slice of the final (H,S,D) output, which replaces the per-expert
 * head gathers and the boolean index-put of `_get_routed_qkv` / `_combine_attn_outputs`
 * (hunyuan.py:612-661, wan.py:388-437).
 *
 * Query side: positions p in [0,n_q) are cut into groups of q_group_len (0 = one group); a workgroup
 * never straddles a group.  Position p reads/writes row  q_rows ? q_rows[y*q_rows_stride_h + p]
 * : q_row_offset + p.  Positions p >= q_valid are written as zeros.
 * Key side: group g attends positions j in [0,n_kv) -> row  kv_rows ? kv_rows[y*kv_rows_stride_h +
 * g*kv_rows_stride_g + j] : kv_row_offset + j.
 * Duplicates: if dup_rows, every position p < n_dup_pos additionally writes its output row to rows
 * dup_rows[y*dup_rows_stride_h + p*n_dup + i], i < n_dup (coreset: centre -> dropped margins).
 * Split keys: n_splits > 1 cuts the key range into n_splits chunks computed by separate workgroups into
 * ws_o / ws_ml (float, sizes from vorta_attn_workspace_bytes) and merged by a second kernel; used for the
 * few text-query rows of the sliding expert that attend every key.
 */
typedef struct vorta_attn_args {
  uint32_t struct_size; /* = sizeof(vorta_attn_args) */
  int32_t dtype;        /* vorta_dtype */
  int32_t head_dim;     /* 128 */
  int32_t n_heads;      /* head slots in this launch (upper bound when n_heads_dev is set) */
  vorta_tensor q, k, v, o;
  const int32_t* head_list;   /* [n_heads] or NULL */
  const int32_t* n_heads_dev; /* optional device count: slots >= *n_heads_dev exit at once (sync-free routing) */
  int32_t n_q, q_group_len, q_row_offset, q_valid;
  const int32_t* q_rows;
  int64_t q_rows_stride_h;
  int32_t n_kv, kv_row_offset;
  const int32_t* kv_rows;
  int64_t kv_rows_stride_h, kv_rows_stride_g;
  const int32_t* dup_rows;
  int64_t dup_rows_stride_h;
  int32_t n_dup_pos, n_dup;
  float scale;        /* softmax scale, 1/sqrt(D) in the reference */
  int32_t block_rows; /* query rows per workgroup: 0 = auto, 128 or 256 */
  int32_t n_splits;   /* >= 1 */
  float* ws_o;        /* [n_heads][n_splits][n_q][D]   when n_splits > 1 */
  float* ws_ml;       /* [n_heads][n_splits][n_q][2]   when n_splits > 1 */
  /* optional device-resident lengths (e.g. L = attention_mask.sum(), hunyuan.py:169, without the host sync):
   * effective n_kv = clamp(*n_kv_dev, 1, n_kv), effective q_valid = min(*q_valid_dev, q_valid) */
  const int32_t* n_kv_dev;
  const int32_t* q_valid_dev;
  /* variant 2 addresses K/V rows with 32-bit offsets: row < 2^24, row_stride_bytes < 2^24 and
   * row * row_stride_bytes < 2^31 for every key row of a head (checked for contiguous ranges, VORTA_EUNSUPPORTED;
   * guaranteed by the caller for kv_rows tables).  Variant 1 has no such limit. */
  int32_t variant; /* kernel body: 0 = auto = 2; 1 = plain (attn_fwd_kernel<T,NW>), 2 = software-pipelined, scores one
                      key block ahead, K/V tiles by LDS-DMA, softmax folded into the score MFMA
                      (attn_fwd_pipe_kernel<T,NW,KVTAB>) */
  int32_t reserved;
  /* Optional query groups of DIFFERENT lengths (ABI 2): one row per workgroup, device int32 [n_q_blocks][3] =
   * (group g, first position, end position) with end - first <= block_rows (which must then be given, 128 or 256).
   * q_group_len is ignored; group g still reads the key list kv_rows + g*kv_rows_stride_g.  Used by the sliding-tile
   * expert: query tiles whose clamped windows coincide (sliding_attn_flex.py:118-120 clamps the window centre, so the
   * two outermost tiles of a dimension see the same keys) are merged into one group, and the group is cut into full
   * workgroups instead of every 792-token tile ending in a 24-row one.  With n_splits > 1 the rows must cover every
   * position in [0, n_q): the split-key merge writes each of them. */
  const int32_t* q_block_table;
  int32_t n_q_blocks;
  int32_t reserved2;
} vorta_attn_args;

int vorta_attn_fwd(const vorta_attn_args* args, void* hip_stream);
#define VORTA_MAX_FUSED_LAUNCHES 6 /* (was 4 before round 4; more -> VORTA_EINVAL) */
/* Up to VORTA_MAX_FUSED_LAUNCHES launches fused into ONE grid (the experts of a routed layer, hunyuan.py:564-591, the text
 * queries of the sliding-tile expert, and -- under sequence parallelism -- up to two full-attention heads that compute
 * only a range of their queries on this rank: q_rows = a slice of the row map, n_heads = 1): workgroups are
 * dispatched in argument order -- pass the longest key loops first -- so one expert's tail is filled by the next
 * expert instead of idling until a kernel boundary.  Every entry must resolve to the 256-row pipelined kernel
 * (VORTA_EUNSUPPORTED otherwise: launch those separately); split-key entries get their merge kernels after. */
int vorta_attn_fwd_batch(const vorta_attn_args* args, int32_t n, void* hip_stream);
/* The same fused grid in TICKET ORDER (ABI 9, a pure addition: a binding asks for the two symbols; 16-bit family only).
 * vorta_attn_fwd_batch decodes a block index to a fixed logical workgroup: every XCD computes a fixed eighth of every
 * segment, and the grid ends with its slowest XCD.  Here a workgroup takes a ticket when it starts instead: from its own XCD
 * class's share of the segments in order (the same workgroups in the same order while that share lasts, so one head's K/V
 * still streams through one L2), then from the class with the most left.  What a logical workgroup computes and writes is
 * unchanged, so outputs are bit-identical to vorta_attn_fwd_batch.
 * The grid is launched with an eighth more blocks than it has logical workgroups (rounded up to a multiple of 8; a profiler
 * shows that size): the hardware deals blocks to the XCDs round-robin whatever their load, so only spare blocks let an XCD
 * that is done early take over work.  A block that finds every counter exhausted exits at once.
 * `tickets`: device memory, vorta_attn_ticket_workspace_ints() int32 (8 per segment + 8), 4-byte aligned, owned by the caller
 * and used by ONE grid at a time (one workspace per stream).  The call zeroes it with a one-block kernel enqueued on
 * `hip_stream` in front of the grid -- under stream capture a node of the graph, so a replay starts from zero too; nothing
 * synchronises with the host.  NULL: exactly vorta_attn_fwd_batch. */
int vorta_attn_fwd_batch_tickets(const vorta_attn_args* args, int32_t n, int32_t* tickets, void* hip_stream);
int vorta_attn_ticket_workspace_ints(void);
/* the launch shape vorta_attn_fwd would use: query rows per workgroup (128 -> kernel attn_fwd_kernel<T,4>,
 * 256 -> attn_fwd_kernel<T,8>) and the number of workgroups; pure host computation */
int vorta_attn_plan(const vorta_attn_args* args, int32_t* block_rows, int64_t* n_workgroups, int32_t* kernel_id);
/* kernel_id = waves*16 + (pipelined ? 1 : 0) + (pipelined with kv table ? 2 : 0):
 *   attn_fwd_kernel<T,NW> (plain) or attn_fwd_pipe_kernel<T,NW,KVTAB> */
/* bytes of ws_o and ws_ml for a given launch (0,0 when n_splits <= 1) */
int vorta_attn_workspace_bytes(const vorta_attn_args* args, uint64_t* ws_o_bytes, uint64_t* ws_ml_bytes);

/*
 * vorta_attn_bwd (ABI 9) -- the gradient of exactly what ONE vorta_attn_fwd launch computes, for the same argument block (16-bit,
 * head_dim 128).  The reference differentiates its experts with torch autograd (`_step_attention` hunyuan.py:136-189, `_attn`
 * wan.py:103-149; the coreset pool / unpool of hunyuan.py:410-457, wan.py:243-270; the sliding tile of hunyuan.py:459-507,
 * wan.py:272-294): this is the derivative of those lines, with the row tables as constants (coreset_select.py ranks with
 * argsort: no gradient flows through the selection there either).  For head slot y, group g, query position p (row r(p)
 * through q_rows / q_row_offset) and keys j < n_kv_eff (rows through kv_rows / kv_row_offset):
 *     dO_eff[p] = w[head] (d_o[r(p)] + sum_i d_o[dup_rows[y][p][i]])     (duplicates: p < n_dup_pos; w = 1 without do_scale)
 *     dO_eff[p] = 0  for p >= q_valid_eff                                 (the forward wrote zeros there)
 *     P = softmax_j(scale q.k)       delta[p] = dO_eff[p] . o[r(p)] = sum_j P[p][j] (dO_eff[p] . v[j])
 *     (fwd.o = the forward's OUTPUT, with d_o's geometry.  The kernel takes delta in the second form, from the P and dP it
 *     forms anyway: sum_j dS[p][j] then cancels to the rounding of those numbers, and a row with a single key gets dS = 0
 *     exactly, as float64 autograd does -- the first form leaves a 1e-7 residue.  fwd.o is validated and not read.)
 *     dv[j] += sum_p P[p][j] dO_eff[p]          dS = P (dO_eff . v[j] - delta[p])
 *     dq[r(p)] += scale sum_j dS[p][j] k[j]     dk[j] += scale sum_p dS[p][j] q[r(p)]
 * dq / dk / dv are fp32 (H,S,D) buffers that are ADDED to (the caller zeroes them): the three experts of the soft mixture
 * add into the SAME buffers and vorta_cast_grads rounds once.  Rows and heads the launch does not name receive nothing.
 * One kernel for every expert (csrc/attn_bwd.hip): query-major 128-row workgroups, the softmax statistics recomputed in a
 * first pass over the keys.  fwd.head_list, n_heads_dev, q_rows, q_group_len, q_block_table, kv_rows (both strides), dup_rows,
 * q_valid, n_kv, n_kv_dev, q_valid_dev and scale mean what they mean for the forward; fwd.n_splits, ws_o, ws_ml and variant
 * are ignored (splitting keys changes nothing in the gradient); fwd.block_rows is only validated (0, 128, 256; the table
 * rows of a q_block_table are cut into 128-row workgroups).
 * REPRODUCIBILITY: dq is written by one workgroup per row (read-add-write; launches on one stream are ordered) and is
 * bit-reproducible; dk and dv are accumulated with vector float atomics (many query blocks touch one key row), so their
 * summation order, and with it their last bits, change from run to run.
 * VORTA_EUNSUPPORTED for a dtype other than bf16 / fp16 or head_dim != 128; VORTA_EINVAL for null or misaligned tensors
 * (16-byte aligned rows: 8 elements of d_o, 4 floats of dq / dk / dv).
 */
typedef struct vorta_attn_bwd_args {
  uint32_t struct_size;       /* = sizeof(vorta_attn_bwd_args) */
  int32_t reserved;
  vorta_attn_args fwd;        /* the forward launch; fwd.o = the forward's OUTPUT (read) */
  vorta_tensor d_o;           /* 16-bit, geometry of fwd.o */
  const void* do_scale;       /* optional [..][do_scale_stride_h] in fwd.dtype, indexed by the HEAD id: w[head] */
  int64_t do_scale_stride_h;  /*   (soft mixture: scores + e, stride 3) */
  vorta_tensor dq, dk, dv;    /* fp32, strides in elements; ADDED to -- the caller zeroes them */
} vorta_attn_bwd_args;

int vorta_attn_bwd(const vorta_attn_bwd_args* args, void* hip_stream);

/*
 * vorta_attn_bwd_stats + vorta_attn_bwd_kmajor (ABI 9, added after the other backward entry points) -- the SAME gradient as
 * vorta_attn_bwd by a second, KEY-MAJOR algorithm, in two launches on one stream:
 *   1. vorta_attn_bwd_stats (csrc/attn_bwd_stats.hip; query-major, no atomics) writes, for every head slot y and query
 *      position p of the launch, two floats to the caller's workspace stats[y * stats_stride_h + 2 p + 0..1]:
 *          lse2[p]  = m c + log2(l)     the log-sum-exp of the row's scores in the exp2 domain, c = scale log2(e)
 *          delta[p] = sum_j P[p][j] (dO_eff[p] . v[j])
 *      with dO_eff as above (do_scale weight, dup_rows gradients added, zero for p >= q_valid_eff).  Positions p >= q_valid_eff
 *      get delta = 0 and a finite lse2.  bwd.dq / dk / dv are not read by this entry point.
 *   2. vorta_attn_bwd_kmajor (csrc/attn_bwd_kmajor.hip) reads them: one workgroup owns 256 keys of one (head slot, group) key
 *      list, keeps their dK and dV on chip while it sweeps the group's queries in 32-row slices, and adds only dQ across
 *      workgroups -- a quarter of the atomic bytes of the query-major kernel, whose time is bounded by them.
 * bwd means what it means for vorta_attn_bwd, including "ADDED to, the caller zeroes" and "rows and heads the launch does not
 * name receive nothing".  n_key_lists = the number of groups (key lists) the rows of a q_block_table refer to (required with a
 * table: the grid has one workgroup per list and key block); 0 without a table, where q_group_len gives it.  The grid is sized
 * from n_kv; *n_kv_dev trims it as in the forward, max(1, min(*n_kv_dev, n_kv)).
 * REPRODUCIBILITY: dq, dk and dv are ALL accumulated with vector float atomics here (dq: one add per key block; dk / dv: one add
 * per workgroup -- key lists of different groups overlap, and the experts of the mixture share the buffers), so none of them
 * is bit-reproducible from run to run.  There is no protocol between workgroups: none ever waits for another.
 * VORTA_EINVAL for a wrong struct_size (either block), a null or misaligned tensor (stats: 8-byte aligned, stats_stride_h even
 * and >= 2 n_q), a table without n_key_lists; VORTA_EUNSUPPORTED for a dtype other than bf16 / fp16 or head_dim != 128;
 * n_heads == 0 is VORTA_OK and launches nothing.
 */
typedef struct vorta_attn_bwd_kmajor_args {
  uint32_t struct_size;    /* = sizeof(vorta_attn_bwd_kmajor_args) = vorta_attn_bwd_kmajor_args_size() */
  int32_t n_key_lists;     /* 0 = from q_group_len */
  vorta_attn_bwd_args bwd; /* the launch, as for vorta_attn_bwd */
  float* stats;            /* [n_heads][stats_stride_h]: written by _stats, read by _kmajor */
  int64_t stats_stride_h;  /* floats per head slot, >= 2 n_q */
} vorta_attn_bwd_kmajor_args;

int vorta_attn_bwd_stats(const vorta_attn_bwd_kmajor_args* args, void* hip_stream);
int vorta_attn_bwd_kmajor(const vorta_attn_bwd_kmajor_args* args, void* hip_stream);
int vorta_attn_bwd_kmajor_args_size(void); /* (vorta_sizeof keeps its 17 indices: a library without these entry points lacks the symbol) */

/*
 * vorta_attn_bwd_dq + vorta_attn_bwd_dkv (ABI 9, a pure addition: no new struct, no new vorta_sizeof index; a binding asks for
 * the two symbols) -- the SAME gradient as vorta_attn_bwd by a third, DETERMINISTIC algorithm: no float atomic anywhere and no
 * protocol between workgroups.  Both take the argument block of the key-major backward, with bwd, stats, stats_stride_h and
 * n_key_lists as described there, and both read the statistics vorta_attn_bwd_stats wrote for the SAME launch earlier on the
 * same stream:
 *   1. vorta_attn_bwd_stats, as above.
 *   2. vorta_attn_bwd_dq (csrc/attn_bwd_dq.hip): query-major, the statistics pass's grid -- a workgroup owns 128 query
 *      positions, sweeps the group's keys once and adds scale dQ to its dq rows with a plain read-add-write, one workgroup
 *      per row as in vorta_attn_bwd.  It reads bwd.dq only: bwd.dk / bwd.dv are neither validated nor touched.
 *   3. vorta_attn_bwd_dkv (csrc/attn_bwd_dkv.hip): the key-major sweep without its dQ half -- a workgroup owns 256 keys of
 *      one (head slot, key list), keeps their dK and dV on chip over the list's queries and adds them to the dk / dv rows
 *      with a plain read-add-write.  It issues ONE KERNEL LAUNCH PER KEY LIST -- n_key_lists launches with a table, the
 *      number of groups without one -- on hip_stream, in list order; each has one workgroup per (head slot, 256-key block).
 *      It reads bwd.dk and bwd.dv only: bwd.dq is neither validated nor touched.
 * The buffers are ADDED to (the caller zeroes them); rows and heads the launch does not name, and query positions at or past
 * q_valid_eff, receive nothing.
 * PRECONDITION (of _dkv; every table this project builds meets it): the first n_kv_eff rows of any ONE key list are distinct,
 * and head_list names distinct heads -- inside one launch every (head, key row) then has a single writer.  Rows that
 * DIFFERENT key lists share (the overlapping windows of the sliding tile), and the launches of the mixture's experts into the
 * same buffers, are summed in stream order.  _dq needs what vorta_attn_bwd needs: no dq row named by two positions.
 * REPRODUCIBILITY: dq, dk and dv are bit-reproducible from run to run: no atomic in either kernel, one writer per row inside
 * a launch with a fixed summation order of its own, and stream order between launches.
 * Error codes as for vorta_attn_bwd_kmajor, except that _dq requires a valid dq only and _dkv a valid dk and dv only (looked
 * at before anything is launched, also when n_heads == 0, which is VORTA_OK and launches nothing).
 */
int vorta_attn_bwd_dq(const vorta_attn_bwd_kmajor_args* args, void* hip_stream);
int vorta_attn_bwd_dkv(const vorta_attn_bwd_kmajor_args* args, void* hip_stream);

/*
 * fp8 (e4m3) path -- BASELINE.json configs[4] "fp8 MFMA QK^T/PV path".  The reference has no fp8 code: this path serves
 * the same three experts (wan.py:243-294, hunyuan.py:410-507) with both contractions on
 * v_mfma_f32_32x32x64_f8f6f4 (2x the bf16 MFMA rate).  Two steps:
 *
 * vorta_fp8_quantize_qkv -- one pass over post-RoPE q,k,v (16-bit, (H,S,D) views) that writes e4m3 copies:
 *     q8 = e4m3( q * qmul[h] ),  k8 = e4m3( k * kmul[h] ),  v8 = e4m3( v * vmul[h][d] )
 *   qmul[h] * kmul[h] = qk_scale * log2(e): the softmax scale and the exp2 conversion are folded into the operands,
 *   so q8 . k8 is the score in the exp2 domain and the kernel's softmax needs no multiply.  The split between q and k
 *   only BALANCES their ranges: t = sqrt(amax_k / (c0 * amax_q)), qmul = c0 * t, kmul = 1 / t, which puts both maxima near
 *   sqrt(c0 * amax_q * amax_k) -- a factor of ~250 inside e4m3's range (448) for unit-variance data, and the format's
 *   relative precision (2^-4) does not depend on where in the normal range a value sits -- so amax_q / amax_k are taken
 *   over a SAMPLE of ~1024 evenly spaced tokens of the head (the tokens that define the key centre, below) instead of a
 *   pass over q and k; values are clamped to +-448 before the conversion in any case.  v is scaled per head and channel
 *   to amax -> 240 with amax over EVERY token (one pass over v: its target sits just under the format's maximum);
 *   v_descale[h][d] = amax_v[h][d] / 240 is applied to the output row in the attention epilogue.
 *   Enqueues 4 launches (sample, abs-max of v, scales, convert); nothing is read back to the host.
 *
 * vorta_attn_fwd_fp8 / _batch_fp8 -- vorta_attn_fwd / _batch with q,k,v = e4m3 (args->dtype = VORTA_FP8E4M3, strides
 *   in BYTES = elements, rows 16-byte aligned); `scale` is ignored (folded, above); the probabilities are re-packed
 *   to e4m3 as P * 2^p_bias with a running reference point at most `defer` below the row max (p_bias + defer <= 8, so
 *   P * 2^p_bias <= 256 < 448); row sums come from one more MFMA against a ones tile (the same rounded P that
 *   multiplies V); the output (ext->out_dtype, bf16 / fp16) is o[d] * v_descale[head][d] / rowsum.
 *   Every other field of vorta_attn_args means what it means for vorta_attn_fwd (row tables, groups, duplicates,
 *   split keys, device-resident lengths).
 *   ext->flags bit1 selects the mixed-precision kernel (csrc/attn_fwd_mx.hip): 16-bit q k^T, e4m3 P V -- see the field.  Since
 *   ABI 7 that kernel writes its probabilities with ONE POWER-OF-TWO SCALE PER QUERY ROW AND 32 KEYS (the block scale of the
 *   P V MFMA's B operand), as vorta_attn_fwd_i8 does: per tile e = rint(max(max c + 64, 0) - 72) for c = score - reference +
 *   p_bias, probability = e4m3(2^(c - e)) 2^e (round to nearest even, subnormals kept); the reference point is the row's first
 *   block's maximum and moves only when a tile lies more than `defer` binades above it (default 24, 0 ... 40).  Nothing is
 *   flushed for lying far below the row's maximum; the all-e4m3 kernel (flags bit1 clear) keeps the single range above.
 */
typedef struct vorta_fp8_quant_args {
  uint32_t struct_size;
  int32_t dtype;            /* input dtype: VORTA_BF16 / VORTA_FP16 */
  int32_t head_dim, heads;  /* 128, H */
  int32_t n_tokens;         /* rows of every head to convert */
  float qk_scale;           /* softmax scale (1/sqrt(D) in the reference) */
  vorta_tensor q, k, v;     /* inputs, (H,S,D) views, strides in elements */
  vorta_tensor q8, k8, v8;  /* outputs, e4m3, strides in bytes; rows 16-byte aligned */
  float* v_descale;         /* [heads][head_dim] out */
  float* ws;                /* workspace, vorta_fp8_quant_ws_floats(heads, head_dim) floats: abs-max slots, multipliers, centres */
  int32_t flags;            /* bit0: v scaled per head instead of per (head, channel);
                               bit1: centre the keys -- k8 = e4m3((k - c[h]) * kmul[h]) with c[h][:] the mean of ~1024 evenly
                               spaced key rows of the head (softmax does not change when one vector is subtracted from
                               every key; the e4m3 error of q8 . k8 shrinks with |k|) */
  int32_t seg_len;          /* 0: q,k,v,q8,k8,v8 are (heads, n_tokens, D) views.  > 0: they are row arrays of n_tokens rows
                               (stride_h unused) in which row r belongs to head (r / seg_len) % heads -- the Ulysses
                               receive layout (vorta_seq_row_map); every head gets its own scales and centre */
  int32_t tail_first;       /* seg_len > 0 and either field non-zero: from row tail_first (a multiple of seg_len) on, only */
  int32_t tail_len;         /* the first tail_len rows of a segment hold data (text rows); the others are skipped
                               (tail_len = 0: the tail region is empty).  A head's tokens are its rows of the segments
                               before tail_first, in order, then its tail rows: the centre of flags bit1 samples the same
                               TOKENS in both layouts, so a head converts to the same bytes on one GPU and on a rank of P */
  int32_t slot_first;       /* seg_len > 0: convert only the rows of head slots [slot_first, slot_first + slot_count) -- the */
  int32_t slot_count;       /* slot group whose exchange has landed while the next one is in flight (0, 0 = every slot).
                               Scales and centres are per head, so converting slot group by slot group gives the bytes
                               one call over all slots gives */
  int32_t video_tokens;     /* seg_len == 0: tokens [0, video_tokens) of a head's sequence are its video tokens, the rest its
                               tail (text) tokens; 0 = all of them.  The sample of flags bit1 and of the q/k abs-max is summed
                               in 8 equal ranges of the video tokens + the tail, so pass the same value wherever the same
                               heads are converted (the segmented layout derives it from tail_first) */
  int32_t token_offset;     /* seg_len == 0, sequence shards (flags bit3 / bit4): the views hold tokens [token_offset, */
  int32_t total_tokens;     /* token_offset + n_tokens) of heads whose whole sequence has total_tokens tokens (0: the views
                               are the whole sequence) */
  const int32_t* src_map;   /* seg_len == 0, optional: q8 / k8 / v8 head h <- head src_map[h] of q / k / v, with that head's
                               scales and centre (the heads in destination order for the exchange); `heads` entries, a
                               negative one = that output head is not written */
} vorta_fp8_quant_args;
/* flags bit2: q and k only -- v, v8 and v_descale are not touched (v arrived as e4m3: vorta_fp8_v_convert on the sender)
 * flags bit3: statistics only -- the sample partials of the tokens this call holds go to their slots of `ws`, nothing is
 *             converted.  Zero the partial region first (vorta_fp8_quant_ws_partials), call once per piece of the sequence
 *             (a shard must hold whole eighths of the video tokens: token_offset and token_offset + n_tokens each equal to
 *             floor(b video_tokens / 8) for some b, or to total_tokens -- anything else is VORTA_EINVAL, a cut chunk would be
 *             summed by nobody; the tail tokens in a call of their own or behind the last eighth), ADD the regions of all
 *             ranks (disjoint slots: exact);
 * flags bit4: no statistics -- multipliers and centres from the partials already in `ws`, then the conversion of the tokens
 *             this call holds.  bit3 calls + all-reduce + bit4 calls write the bytes ONE plain call over the assembled
 *             sequence writes: the send side of the Ulysses exchange moves q and k as e4m3 (vorta/ulysses/utils.py:61-91
 *             moves them in 16 bits). */
int vorta_fp8_quant_ws_partials(int32_t heads, int32_t head_dim, int64_t* first_float, int64_t* n_floats);

int vorta_fp8_quant_ws_floats(int32_t heads, int32_t head_dim);
int vorta_fp8_quantize_qkv(const vorta_fp8_quant_args* args, void* hip_stream);

/*
 * V on its own, for the sender side of the Ulysses exchange (vorta/ulysses/utils.py:61-91 moves 16-bit q, k, v): each rank
 * takes the per-(head, channel) abs-max of ITS sequence shard of v (vorta_fp8_v_absmax: amax[h][d] is raised atomically,
 * the caller zeroes it first; several calls accumulate -- video rows, then the replicated text rows), the ranks
 * all-reduce amax with MAX (heads x 128 floats), and vorta_fp8_v_convert writes the e4m3 shard with the scales of the
 * whole sequence, heads already in destination order (v8 head h <- v head src_map[h]): v crosses the links at half the
 * bytes and lands as the attention kernels read it.  The bytes and v_descale equal what vorta_fp8_quantize_qkv produces
 * from the assembled 16-bit sequence (abs-max over shards = abs-max over the sequence).
 */
typedef struct vorta_fp8_v_args {
  uint32_t struct_size;
  int32_t dtype;            /* input dtype: VORTA_BF16 / VORTA_FP16 */
  int32_t head_dim, heads;  /* 128; heads of v (absmax) / of v8 (convert) */
  int32_t n_tokens;
  int32_t flags;            /* bit0: one scale per head instead of per (head, channel) */
  vorta_tensor v;           /* (H, n_tokens, D) view, strides in elements */
  vorta_tensor v8;          /* convert: (heads, n_tokens, D) e4m3 out, strides in bytes */
  const int32_t* src_map;   /* convert: [heads] source head of every destination head, or NULL (identity) */
  float* amax;              /* [H][D], indexed by the SOURCE head: absmax raises it, convert reads it */
  float* v_descale;         /* convert: optional out [heads][D], indexed by the DESTINATION head: amax / 240 */
} vorta_fp8_v_args;

int vorta_fp8_v_absmax(const vorta_fp8_v_args* args, void* hip_stream);
int vorta_fp8_v_convert(const vorta_fp8_v_args* args, void* hip_stream);

typedef struct vorta_attn_fp8_ext {
  uint32_t struct_size;
  int32_t out_dtype;           /* VORTA_BF16 / VORTA_FP16: element type of args->o */
  const float* v_descale;      /* [..][head_dim], indexed by the head id (not the slot) */
  int64_t v_descale_stride_h;  /* floats between heads (head_dim) */
  float p_bias;                /* log2 bias of the e4m3 probabilities; 0 = default (5) */
  float defer;                 /* deferred-rescale threshold in log2 units; 0 = default (3; mixed kernel: 24); p_bias + defer <= 8
                                  (mixed kernel: 0 <= defer <= 40, p_bias <= 16) */
  int32_t flags;               /* bit0: row sums by VALU adds of the unrounded P instead of the ones-tile MFMA;
                                  bit1 (ABI 4): MIXED precision -- q, k (and o) are 16-bit tensors of type args->dtype =
                                  out_dtype with strides in elements, the scores run on the 16-bit MFMA with args->scale
                                  folded as in vorta_attn_fwd; only v is e4m3 (strides in bytes, vorta_fp8_v_absmax /
                                  vorta_fp8_v_convert or the v half of vorta_fp8_quantize_qkv) and only P is packed to
                                  e4m3.  The score is where an 8-bit mantissa costs: the all-e4m3 path holds 40 dB against
                                  the 16-bit kernels only where the softmax is flat, this one 42-70 dB on every input
                                  family tried, at 1.2 x the 16-bit rate instead of 1.7 x */
  int32_t reserved;
} vorta_attn_fp8_ext;

int vorta_attn_fwd_fp8(const vorta_attn_args* args, const vorta_attn_fp8_ext* ext, void* hip_stream);
int vorta_attn_fwd_batch_fp8(const vorta_attn_args* args, const vorta_attn_fp8_ext* ext, int32_t n, void* hip_stream);

/*
 * Int8 scores (ABI 6; BASELINE.json configs[4], no reference counterpart: the reference computes the three experts of
 * wan.py:243-294 / hunyuan.py:410-507 in the dtype of q, k, v).  precision "i8pv": q k^T on v_mfma_i32_32x32x32_i8 (the
 * e4m3 MFMA rate) with 7 bits next to the operand's maximum -- the all-e4m3 path loses 40 dB on peaked or outlier-carried
 * logits because e4m3 has 3 mantissa bits wherever a value sits -- and P V in e4m3 as in the mixed kernel.
 * With cq, ck the per-head means of q and k (from ~1024 sampled tokens) and s a per-channel balance vector,
 *     q . k  =  (q - cq) . (k - ck)  +  cq . (k - ck)  +  (a term that does not depend on the key: softmax does not see it)
 *            =  [(q - cq) s] . [(k - ck) / s]  +  b[key]
 * the first product runs in int8 (both operands centred: no common component eats the 8 bits; channel ranges balanced, which
 * is what a FIXED-point format needs when a few qk-norm channels carry the logits), b[key] is computed in float32 and enters
 * the int32 accumulator as its initial value.
 *
 * vorta_i8_quantize_k -- per head h, from ~1024 evenly spaced tokens (the same tokens in the (H,S,D) view and in the segmented
 *   Ulysses receive layout): ck[d] = mean k, cq[d] = mean q, s[d] = clamp((var k[d] / var q[d])^(1/4), 1/8, 8).  Then over every
 *   row of the head:   kt = (k - ck) / s      amax[h] = max |kt|  (exact, over all rows)      sk[h] = amax[h] / 127
 *                      k8[row][d] = rint(kt 127 / amax[h])          k_bias[row] = (cq . (k - ck)) 127 / amax[h]
 *   Outputs: k8 (int8 rows of head_dim bytes), k_bias (one float per row: b[key] in units of sk[h]), q_prep (heads x 2 x
 *   head_dim floats: cq then s -- what the attention kernel applies to its query rows before quantising them itself) and
 *   k_head_scale = sk (heads floats).
 */
typedef struct vorta_i8_quant_args {
  uint32_t struct_size;
  int32_t dtype;            /* input dtype: VORTA_BF16 / VORTA_FP16 */
  int32_t head_dim, heads;  /* 128, H */
  int32_t n_tokens;         /* rows of every head (seg_len == 0) or of the row array (seg_len > 0) */
  vorta_tensor q, k;        /* inputs, strides in elements; q is only sampled (centre and balance statistics) */
  vorta_tensor k8;          /* out: int8, strides in bytes, rows 16-byte aligned; same head / row geometry as k */
  float* k_bias;            /* out: k_bias[h * k_bias_stride_h + row]  (seg_len > 0: k_bias[row]) */
  int64_t k_bias_stride_h;
  float* q_prep;            /* out [heads][2][head_dim]: cq | s */
  float* k_head_scale;      /* out [heads]: sk */
  float* ws;                /* workspace, 2 * heads * head_dim + heads floats: ck | 1 / s | amax */
  int32_t flags;            /* bit0: no balancing (s = 1); bit1: no centring (ck = cq = 0, k_bias = 0) */
  int32_t seg_len;          /* as vorta_fp8_quant_args: 0 = (heads, n_tokens, D) views; > 0 = one row array, row r belongs to */
  int32_t tail_first;       /* head (r / seg_len) % heads, tail (text) rows from tail_first on, tail_len per segment */
  int32_t tail_len;
  int32_t slot_first;       /* seg_len > 0: only head slots [slot_first, slot_first + slot_count) (0, 0 = all) */
  int32_t slot_count;
} vorta_i8_quant_args;

int vorta_i8_quantize_k(const vorta_i8_quant_args* args, void* hip_stream);

/*
 * ABI 8 -- per-head choice between the int8-score kernel and the mixed-precision one ("auto8" of the Python host): int8 scores
 * with ONE key scale per head resolve the bulk of a heavy-tailed head's keys to 0 / +-1 (Student-t(3): abs-max ~ 250 sigma over
 * 10^7 samples; relative error 0.10-0.19 where every other input family tried stays under 0.07).
 * vorta_i8_tail_flags: flags[h] = 1 when the root mean square of head h's int8 keys (k8 of vorta_i8_quantize_k, (heads,
 *   n_tokens, head_dim) view, strides in bytes) over ~1024 evenly spaced tokens is below `min_rms` counts, else 0; row_map (NULL:
 *   token = row) gives the row of each token inside a head's view (the Ulysses receive layout).  Exact integer arithmetic: the
 *   flag is reproducible, and the same under sequence parallelism.
 * vorta_split_heads: list0 / list1 = the heads of head_list[0 .. n) (NULL: 0 .. n-1; n = min(*n_heads_dev, n_heads) when
 *   n_heads_dev is given) whose flag is 0 / 1, order kept; counts[0], counts[1] = their lengths.  The two lists (room for
 *   n_heads entries each) and the counts (device) are what vorta_attn_args.head_list / n_heads_dev of the two launches take:
 *   a launch over an empty list exits in its first instruction.  No host synchronisation anywhere.
 */
int vorta_i8_tail_flags(const vorta_tensor* k8, int32_t heads, int32_t n_tokens, const int32_t* row_map, float min_rms, int32_t* flags,
                        void* hip_stream);
int vorta_split_heads(const int32_t* head_list, const int32_t* n_heads_dev, int32_t n_heads, const int32_t* flags,
                      int32_t* list0, int32_t* list1, int32_t* counts, void* hip_stream);

/*
 * vorta_attn_fwd_i8 -- the gather flash-attention of vorta_attn_fwd with int8 scores and e4m3 P V.
 *   args->q: 16-bit (args->dtype), strides in elements.  Every WAVE takes its 32 query rows, qt = (q - cq) s with the head's
 *            q_prep, the abs-max over the 32 rows (sq = amax / 127) and rounds them to int8 itself -- queries are read once
 *            per workgroup; a wave whose abs-max is below 2^-12 (every row on the head's centre) takes q8 = 0, sq = 1: its scores are
 *            the bias term alone;
 *   args->k: the int8 rows of vorta_i8_quantize_k, strides in BYTES; k_bias its per-row floats (indexed like k rows:
 *            head * k_bias_stride_h + row, through kv_rows when given); k_head_scale[head] = sk;
 *   args->v: e4m3 (vorta_fp8_v_absmax / vorta_fp8_v_convert), strides in bytes, with v_descale as in vorta_attn_fp8_ext;
 *   args->o: 16-bit (args->dtype).
 *   score of (query i of wave w, key j) in the exp2 domain = u (q8[i] . k8[j] + rint(k_bias[j] / sq[w])), u = scale log2(e)
 *   sq[w] sk[head] (the int32 accumulator starts from the rounded bias; |bias| is clamped to 2 000 000 units).
 *   Probabilities: P' = 2^(score - reference + p_bias) against the row's reference point (its first block's maximum; it moves
 *   only when a later block lies more than `defer` binades above it), written to e4m3 by ONE conversion instead of exp2 +
 *   round, with ONE POWER-OF-TWO SCALE PER QUERY ROW AND 32 KEYS (ABI 7): for y = 8 log2 P' + 56 and e = max(rint((max y over
 *   the 32 consecutive keys of one half of the 64-key block - 120) / 8), -100), the byte is rint(y - 8 e) (v_cvt_pk_u8_f32, saturating at 0:
 *   the e4m3 number whose exponent field is the integer part of log2 P' - e and whose mantissa is the LINEAR interpolation of
 *   its fraction, +-3 % of 2^x) and 2^e is the block scale of the P V MFMA's B operand (v_mfma_scale_f32_32x32x64_f8f6f4).
 *   The range of a probability is the scale's, not e4m3's: nothing is flushed for lying far below the ROW's maximum (up to ABI
 *   6 everything below 2^-14 ... 2^-11
 *   of it was).  Tables, groups, duplicates, split keys and the fused grid as vorta_attn_fwd_fp8.
 */
typedef struct vorta_attn_i8_ext {
  uint32_t struct_size;
  int32_t flags;               /* reserved, 0 */
  const float* k_bias;
  int64_t k_bias_stride_h;     /* floats between heads of k_bias */
  const float* q_prep;         /* [..][2][head_dim], indexed by the head id */
  int64_t q_prep_stride_h;     /* floats between heads (2 * head_dim) */
  const float* k_head_scale;   /* [..], indexed by the head id */
  const float* v_descale;      /* [..][head_dim], indexed by the head id */
  int64_t v_descale_stride_h;
  float p_bias, defer;         /* 0 = defaults: p_bias 5 (0 ... 16); defer 24 binades (0 ... 64: P' <= 2^(defer + 9) in fp32) */
} vorta_attn_i8_ext;

int vorta_attn_fwd_i8(const vorta_attn_args* args, const vorta_attn_i8_ext* ext, void* hip_stream);
int vorta_attn_fwd_batch_i8(const vorta_attn_args* args, const vorta_attn_i8_ext* ext, int32_t n, void* hip_stream);

/*
 * vorta_coreset_select -- coreset_select.py:68-124 (ranking part) + :159-166 (scatter destinations).
 *
 * For every head slot and every window group of g = gw[0]*gw[1]*gw[2] tokens of the (t,h,w) latent:
 * cosine similarity (F.normalize eps 1e-12, fp32 arithmetic) between the centre token and each of the
 * g-1 margin tokens, ascending stable rank; the n_keep least similar margins are kept.
 * Writes   keep_rows[y][G*(1+n_keep) (+ n_tail)] : token ids of the packed sequence
 *                    [G centres | G x n_keep kept margins (group-major, least similar first) | tail]
 *          drop_rows[y][G][g-1-n_keep]           : token ids of the dropped margins of each group
 * (tail = n_tail consecutive ids starting at tail_first: the text tokens appended by hunyuan.py:441-444).
 * If row_map is given, every emitted id i is replaced by row_map[i] (physical row of token i: the
 * zero-copy Ulysses layout), while x is still read at row_map[i].
 */
typedef struct vorta_coreset_args {
  uint32_t struct_size;
  int32_t dtype, head_dim, n_heads;
  vorta_tensor x; /* (H,S,D): Q or K */
  const int32_t* head_list;
  const int32_t* n_heads_dev;
  int32_t latent[3], group[3];
  int32_t n_keep; /* kept margins per group = int(g*(1-rate)) - 1 */
  int32_t tail_first, n_tail;
  const int32_t* row_map; /* optional [t*h*w + ...] */
  int32_t* keep_rows;
  int64_t keep_rows_stride_h;
  int32_t* drop_rows; /* may be NULL (K side needs no drop list) */
  int64_t drop_rows_stride_h;
  /* ABI 4: optional second keep list for the KEY side, same length as keep_rows: per group its centre and kept margins
   * together, in ascending token order, groups in order, then the tail -- the same SET of rows as keep_rows in an order
   * that keeps the gathered K/V rows of a tile close in memory (the softmax does not depend on key order; the query
   * side must keep the packed order: positions < G are the centres the duplicate list refers to).  keep_rows may be NULL
   * when only this list is wanted. */
  int32_t* keep_rows_kv;
  int64_t keep_rows_kv_stride_h;
} vorta_coreset_args;

int vorta_coreset_select(const vorta_coreset_args* args, void* hip_stream);
/* Partial geometry (ABI 9, a pure addition): a window `group` that does not divide `latent`.  The windows are the
 * ng = floor(latent / group) whole ones per dimension the reference's get_group_info keeps when it crops
 * (coreset_select.py:36-40), G = prod(ng); the C = S - G*g tokens outside the cropped box stay at full resolution.  Same
 * arguments; the lists are
 *   keep_rows[y][G*(1+n_keep) + C + n_tail] : [G centres | G x n_keep kept margins | C remainder tokens, ascending | tail]
 *   keep_rows_kv                            : its window part as for vorta_coreset_select, then the same remainder and tail
 *   drop_rows[y][G][g-1-n_keep]             : as for vorta_coreset_select (a remainder token is never a duplicate)
 * Two launches on the stream: the selection over the G windows (the kernel of vorta_coreset_select) and one that writes
 * the remainder and tail rows.  VORTA_EINVAL when a dimension holds no whole window.  A dividing geometry gives the lists
 * of vorta_coreset_select. */
int vorta_coreset_select_partial(const vorta_coreset_args* args, void* hip_stream);

/*
 * vorta_sta_build_tables -- sliding_attn_flex.py:72-134 (mask_mod) + tile.py:7-78 (tile/untile) as tables.
 *
 *   q_rows [S]                 tile-major position -> raster token id (tile.py:26-29, sp = 1)
 *   kv_rows[n_tiles][n_kv]     keys visible to each q tile: the clamped window of tiles
 *                              (sliding_attn_flex.py:118-127) in tile-major order, then the t_eff valid
 *                              text tokens S..S+t_eff-1 (:112);  n_kv = prod(min(n_d, ...)) * tok + t_eff
 * n_kv is returned through *n_kv_out (host).  row_map as in vorta_coreset_select.
 */
typedef struct vorta_sta_args {
  uint32_t struct_size;
  int32_t latent[3], tile[3], window[3];
  int32_t t_eff;
  const int32_t* row_map;
  int32_t* q_rows;
  int32_t* kv_rows;
} vorta_sta_args;

int vorta_sta_table_sizes(const vorta_sta_args* args, int32_t* n_tiles, int32_t* tok_per_tile, int32_t* n_kv);
int vorta_sta_build_tables(const vorta_sta_args* args, void* hip_stream);
/* Partial geometry (ABI 9, a pure addition): a tile that does not divide the latent grid.  nt = ceil(latent / tile) tiles
 * per dimension, tile i = [i*tile, min((i+1)*tile, latent)); the window rule of vorta_sta_build_tables on that tile grid.
 *   q_rows [S]                       tile-major position -> token: tiles in raster order, the tokens of a tile in raster
 *                                    order of its own (possibly thinner) box
 *   kv_rows[n_lists][list_stride]    one row per DISTINCT key list.  A list is fixed by the first tile (f0,f1,f2) of the
 *                                    clamped window, f_d in [0, nt_d - cnt_d]; list l = (f0*nf1 + f1)*nf2 + f2.  Its
 *                                    list_n_kv[l] entries are the tokens of the window's tiles (their union is one box,
 *                                    listed in raster order) and then the t_eff text rows; entries behind them repeat the
 *                                    first one.  Lists that hold a thin last tile are shorter: at most 8 lengths.
 * vorta_sta_partial_sizes is host-only; list_n_kv (host, list_n_kv_cap entries, or NULL) receives the lengths.
 * row_map as in vorta_sta_build_tables. */
int vorta_sta_partial_sizes(const vorta_sta_args* args, int32_t* n_tiles, int32_t* n_lists, int32_t* list_stride,
                            int32_t* list_n_kv, int32_t list_n_kv_cap);
int vorta_sta_build_tables_partial(const vorta_sta_args* args, void* hip_stream);

/*
 * vorta_router_route -- vorta/patch/router.py:33-43 (Router.forward) + the top-1 / tau rule of
 * `_get_routed_qkv` (hunyuan.py:620-624, wan.py:396-400), without the host sync of torch.nonzero.
 *
 *   scores[b][h][e] = softmax_e( W[3h+e,:] . silu(temb[b,:]) + bias[3h+e] )           (dtype of temb)
 *   expert_of_head[h] = argmax_e scores[0][h][e]  (first max), 0 if that score < tau   (batch item 0)
 *   head_lists[e][..] / head_counts[e] : ascending heads of expert e (device; feed n_heads_dev)
 */
typedef struct vorta_router_args {
  uint32_t struct_size;
  int32_t dtype;
  int32_t batch, embed_dim, heads, n_experts; /* n_experts = 3 */
  const void* temb;   /* [batch][embed_dim] */
  const void* weight; /* [heads*n_experts][embed_dim] */
  const void* bias;   /* [heads*n_experts] */
  float tau;
  void* scores;            /* [batch][heads][n_experts], may be NULL */
  int32_t* expert_of_head; /* [heads] */
  int32_t* head_lists;     /* [n_experts][heads] */
  int32_t* head_counts;    /* [n_experts] */
  float* ws_logits;        /* workspace [batch][heads][n_experts] floats (caller-owned) */
} vorta_router_args;

int vorta_router_route(const vorta_router_args* args, void* hip_stream);
/* Same dispatch rule applied to scores that already exist (the `routing_score` argument of the processors,
 * hunyuan.py:528): uses temb/weight/bias = NULL, `scores` as INPUT [batch][heads][n_experts], no workspace. */
int vorta_route_scores(const vorta_router_args* args, void* hip_stream);
/* Route plan: the router input is the pure timestep embedding (modeling_hunyuan.py:627-628,
 * modeling_wan.py:215), the same for every block, so all layers' routes are known at the start of a denoising
 * step.  One call (2 launches) for n_layers routers sharing `temb`: every array gains a leading [n_layers]
 * dimension -- weight [L][heads*n_experts][embed_dim], bias [L][heads*n_experts], scores [L][batch][heads][n_experts],
 * expert_of_head [L][heads], head_lists [L][n_experts][heads], head_counts [L][n_experts], ws_logits
 * [L][batch][heads][n_experts].  The reference runs one Router module per block inside the block's forward
 * (modeling_hunyuan.py:491,555; modeling_wan.py:127). */
int vorta_route_plan(const vorta_router_args* args, int32_t n_layers, void* hip_stream);

/*
 * vorta_qk_norm_rope -- the producer step right before the attention boundary, in place:
 * RMSNorm of q or k (hunyuan.py:62-73: per head over D with attn.norm_q / norm_k [diffusers RMSNorm];
 * wan.py:85-89: across all H*D channels of a token, before the head split) followed by the rotary embedding
 * (hunyuan.py:75-104 via diffusers apply_rotary_emb(use_real, unbind_dim=-1); wan.py:34-37 complex product --
 * the same rotation of interleaved pairs).  One read and one write of the tensor instead of ~10 torch passes.
 *   tokens [token_offset, token_offset + n_tokens) of every head are normalised; the first rope_tokens of them
 *   are rotated with cos/sin[token][D] (fp32; NULL = no rotation: text tokens, hunyuan.py:90-102).
 */
typedef struct vorta_norm_rope_args {
  uint32_t struct_size;
  int32_t dtype, head_dim, heads;
  vorta_tensor x;       /* (H,S,D) view, updated in place */
  const void* weight;   /* [D] or, if across_heads, [H*D]; dtype of x; NULL = no scale */
  const float* cos;     /* [n_tokens][D] or NULL */
  const float* sin;
  int32_t n_tokens, token_offset, rope_tokens;
  float eps;
  int32_t across_heads; /* 0: mean over D per head (Hunyuan); 1: mean over H*D per token (Wan) */
} vorta_norm_rope_args;

int vorta_qk_norm_rope(const vorta_norm_rope_args* args, void* hip_stream);

/*
 * vorta_qk_norm_rope_bwd (ABI 9, added after the other backward entry points) -- the gradient of ONE vorta_qk_norm_rope call
 * for the same argument block.  The reference differentiates hunyuan.py:62-104 / wan.py:85-100 with torch autograd; this is
 * the derivative of those lines in one pass.  With y = x r w, r = rsqrt(mean(x^2) + eps) (mean over D, or over H*D when
 * across_heads), out = the interleaved-pair rotation of y, and g = d(out), in fp32:
 *     dy[2i]   = g[2i] cos[2i]     + g[2i+1] sin[2i+1]
 *     dy[2i+1] = g[2i+1] cos[2i+1] - g[2i]   sin[2i]                (rows >= rope_tokens, or no table: dy = g)
 *     dx       = r (w dy) - x r^3 / n sum_n(w dy x)                  (n = D or H*D; w = 1 when weight is NULL)
 *     dweight[c] = sum over the call's rows of dy[c] x[c] r          ([D] or [H*D], float32)
 * fwd.x is the forward's INPUT (pre-norm; read only -- the forward ran in place, so the caller kept a copy).  g and dx are
 * 16-bit (H,S,D) views of fwd.dtype with strides of their own; dx may alias g.  Only tokens [token_offset, token_offset +
 * n_tokens) of dx are written: a caller that covered a tensor with several forward calls (video and text ranges) covers dx
 * with the same calls.  dweight (may be NULL) is OVERWRITTEN by every call -- each call owns only its rows -- and the caller
 * adds the calls' results.  It is deterministic: every workgroup reduces its rows to one fp32 partial per channel in `ws`
 * (caller-owned, ws_floats >= min(ceil(n_tokens / 4), VORTA_NORM_ROPE_BWD_PARTS) * channels floats, 16-byte aligned; only
 * needed with dweight) and a second launch adds the partials in a fixed order; no float atomics.
 * Codes as vorta_qk_norm_rope: head_dim != 128, a dtype other than bf16 / fp16, or more than 40 heads across_heads are
 * VORTA_EUNSUPPORTED; n_tokens == 0 returns VORTA_OK and zeroes dweight when it is given.
 */
#define VORTA_NORM_ROPE_BWD_PARTS 1024
typedef struct vorta_norm_rope_bwd_args {
  uint32_t struct_size; /* = sizeof(vorta_norm_rope_bwd_args) */
  int32_t reserved;
  vorta_norm_rope_args fwd; /* the forward call; fwd.x = the forward's INPUT (read) */
  vorta_tensor g;           /* gradient of the forward's output, fwd.dtype */
  vorta_tensor dx;          /* out, fwd.dtype; may alias g */
  float* dweight;           /* out [D] or [H*D], or NULL */
  float* ws;                /* workspace for dweight's partial sums (NULL without dweight) */
  int64_t ws_floats;
} vorta_norm_rope_bwd_args;

int vorta_qk_norm_rope_bwd(const vorta_norm_rope_bwd_args* args, void* hip_stream);

/*
 * vorta_mix_experts -- the score-weighted sum of the training-time forward:
 *   out[h][row][:] = sum_e scores[h][e] * x[e][h][row][:]        (fp32 accumulation, one rounding)
 * `_combine_attn_outputs`, hunyuan.py:509-513 == wan.py:296-300 (stack + multiply + sum over the expert axis).
 * Its derivative is vorta_mix_experts_bwd (scores) and the do_scale weight of vorta_attn_bwd (expert outputs), below.
 */
typedef struct vorta_mix_args {
  uint32_t struct_size;
  int32_t dtype, head_dim, heads, n_experts; /* n_experts = 3 */
  int32_t n_rows;
  vorta_tensor x[3];   /* (H, n_rows, D) views: outputs of expert 0 / 1 / 2 for ALL heads */
  vorta_tensor out;    /* (H, n_rows, D) view; may alias one of x */
  const void* scores;  /* [heads][n_experts], dtype of x: routing scores of batch item 0 */
} vorta_mix_args;

int vorta_mix_experts(const vorta_mix_args* args, void* hip_stream);

/*
 * vorta_mix_experts_bwd (ABI 9) -- the derivative of `_combine_attn_outputs` (hunyuan.py:509-513 == wan.py:296-300) with
 * respect to the routing scores:
 *     dscores[h][e] = sum_{row,d} d_out[h][row][d] * x[e][h][row][d]            (fp32 out, [heads][3])
 * one pass over d_out and the three saved expert outputs.  Deterministic: VORTA_MIX_BWD_PARTS partial sums per head over fixed
 * row ranges, each a fixed reduction tree, summed in a fixed order by a second launch; no float atomics.  The derivative
 * with respect to expert e's output, scores[h][e] * d_out, is NOT materialised: vorta_attn_bwd takes the weight (do_scale).
 */
#define VORTA_MIX_BWD_PARTS 64
typedef struct vorta_mix_bwd_args {
  uint32_t struct_size;
  int32_t dtype, head_dim, heads, n_experts; /* n_experts = 3 */
  int32_t n_rows;
  vorta_tensor x[3];   /* (H, n_rows, D) views: the saved outputs of expert 0 / 1 / 2 */
  vorta_tensor d_out;  /* (H, n_rows, D) view, dtype of x */
  float* dscores;      /* out [heads][n_experts] */
  float* ws;           /* workspace, heads * VORTA_MIX_BWD_PARTS * 4 floats (caller-owned) */
} vorta_mix_bwd_args;

int vorta_mix_experts_bwd(const vorta_mix_bwd_args* args, void* hip_stream);

/*
 * vorta_cast_grads (ABI 9) -- the one rounding at the end of a backward: up to three fp32 (H, n_rows, D) accumulation buffers
 * (dq, dk, dv of vorta_attn_bwd) -> 16-bit (H, n_rows, D) views, round to nearest even.
 */
typedef struct vorta_cast_args {
  uint32_t struct_size;
  int32_t dtype, head_dim, heads, n_rows, n_tensors; /* dtype of dst: VORTA_BF16 / VORTA_FP16; 1 <= n_tensors <= 3 */
  vorta_tensor src[3]; /* fp32, strides in elements, rows 16-byte aligned */
  vorta_tensor dst[3]; /* 16-bit, strides in elements, rows 16-byte aligned */
} vorta_cast_args;

int vorta_cast_grads(const vorta_cast_args* args, void* hip_stream);

/*
 * vorta_expert_fidelity (ABI 9, a pure addition: a binding asks for the symbol and for vorta_fidelity_args_size(); vorta_sizeof
 * keeps its 17 indices) -- how far the sparse experts and the mixed output are from the full expert, per head, from the three
 * expert outputs the training-time forward already holds (`_combine_attn_outputs`' inputs, hunyuan.py:509-513 == wan.py:296-300;
 * the reference has no such measurement).  With x0 = x[0] (full attention) and t_0 = x[1] (coreset), t_1 = x[2] (sliding tile),
 * t_2 = mixed (the output of vorta_mix_experts; optional), over the head's n_rows x 128 elements:
 *     sq_ref[h]     = sum x0^2                 max_ref[h]    = max |x0|           range_ref[h] = max x0 - min x0   (optional)
 *     sq_err[h][j]  = sum d_j^2                max_err[h][j] = max |d_j|          d_j = fl(t_j - x0)
 * all float32; [h][j] with a stride of 3, and column 2 is WRITTEN ONLY when mixed.ptr is given.  One pass: every row of every
 * buffer is read once, 16 bytes a lane.
 * ARITHMETIC: the values are widened to float32 (exact); fl() is the one float32 rounding of the difference (it is exact
 * whenever the exponents of the two 16-bit values are less than 16 apart; in general |fl(d) - d| <= 2^-24 |d|); squares and sums
 * are float32, maxima are exact maxima of the |fl(d_j)|.  A head with a NaN among its inputs, or an Inf that meets an Inf in a
 * difference, gets NaN in the sums AND the maxima of the columns it reaches, as a float64 evaluation would; other heads are not
 * touched.  Squares below 2^-126 (bf16 differences below 2^-63) underflow: the bound below is for data above that.
 * DETERMINISTIC, in the manner of vorta_mix_experts_bwd: VORTA_FIDELITY_PARTS partials per head over the fixed row ranges
 * [b per, (b + 1) per), per = ceil(n_rows / PARTS); in a partial, a lane owns 8 channels of every 16th row of the range and adds
 * one row's 8 squares as a fixed tree to its running sum; lanes meet by shuffles, the four waves through LDS, the partial goes to
 * the caller's workspace with plain vector stores, and a second launch joins the parts of a head as a fixed shuffle tree.  No
 * float atomic; maxima and minima take the same path.  The same bits on every run and every stream.
 * LONGEST CHAIN of float32 roundings a sum passes through = VORTA_FIDELITY_CHAIN(n_rows):
 *     2 (the rounded difference, squared) + 4 (a row's 8 squares: d^2, one fma, two tree levels) + V (one add per row a lane
 *     visits, V = ceil(per / 16)) + 6 (wave shuffles) + 2 (four waves) + 6 (64 parts) + 1 (so that the LINEAR bound holds:
 *     (1 + u)^n - 1 <= (n + 1) u for n <= 4096)
 * and every term is non-negative, so |sum - exact| <= CHAIN 2^-24 exact.  Hunyuan-129f (119 056 rows): 138, i.e. 8.3e-6; the
 * bound stays under 1e-4 up to 1.69 million rows a head.
 * VORTA_EINVAL for a wrong struct_size, negative sizes, a null or misaligned output (4 bytes) or workspace (16 bytes), a null
 * or misaligned tensor (16-byte aligned rows; a null x is accepted only with n_rows == 0); VORTA_EUNSUPPORTED for a dtype
 * other than bf16 / fp16 or head_dim != 128.  Everything is looked at before anything is launched.  heads == 0 is VORTA_OK and
 * launches nothing; n_rows == 0 is VORTA_OK and writes zeros.
 */
#define VORTA_FIDELITY_PARTS 64
#define VORTA_FIDELITY_WS_FLOATS 12 /* per head and part */
#define VORTA_FIDELITY_CHAIN(n_rows) (((((int64_t)(n_rows) + VORTA_FIDELITY_PARTS - 1) / VORTA_FIDELITY_PARTS + 15) / 16) + 21)
typedef struct vorta_fidelity_args {
  uint32_t struct_size; /* = sizeof(vorta_fidelity_args) = vorta_fidelity_args_size() */
  int32_t dtype, head_dim, heads, n_rows;
  int32_t reserved;
  vorta_tensor x[3];   /* (H, n_rows, D) views, strided like vorta_mix_args.x: outputs of expert 0 / 1 / 2 */
  vorta_tensor mixed;  /* (H, n_rows, D) view, dtype of x; ptr NULL = not given */
  float* sq_ref;       /* out [heads] */
  float* max_ref;      /* out [heads] */
  float* sq_err;       /* out [heads][3] */
  float* max_err;      /* out [heads][3] */
  float* range_ref;    /* out [heads], or NULL (what a PSNR over the data range needs) */
  float* ws;           /* workspace, heads * VORTA_FIDELITY_PARTS * VORTA_FIDELITY_WS_FLOATS floats, 16-byte aligned (caller-owned) */
} vorta_fidelity_args;

int vorta_expert_fidelity(const vorta_fidelity_args* args, void* hip_stream);
int vorta_fidelity_args_size(void);

/*
 * vorta_sampled_fidelity (ABI 9, a pure addition: a binding asks for the symbol and for vorta_sampled_fidelity_args_size();
 * vorta_sizeof keeps its 17 indices) -- how far the output a ROUTED call wrote is from dense attention, per head, on a sample of
 * n_rows query rows: `ref` holds the dense reference rows compactly, `out` is the routed output read in place, rows[p] the
 * physical row of `out` that sample position p names (a caller under sequence parallelism composes it with vorta_seq_row_map's
 * table).  The reference has no such measurement.  For head slot y < n_heads (< *n_heads_dev when given), head h = head_list ?
 * head_list[y] : y, over the n_rows x 128 elements  x0 = ref[h][p][:],  t = out[h][rows[p]][:]:
 *     sq_ref[h] = sum x0^2     max_ref[h] = max |x0|     range_ref[h] = max x0 - min x0 (optional)
 *     sq_err[h] = sum d^2      max_err[h] = max |d|      d = fl(t - x0)
 *     row_sq_err[h * n_rows + p] = the sum of row p's 128 d^2 (optional: where in the clip a head is off)
 * all float32, indexed by the HEAD, not by the slot: heads the launch does not name, and slots at or past *n_heads_dev, keep
 * what the caller's buffers held.  head_list names distinct heads.  Row addresses are 64-bit: head * stride_h + rows[p] *
 * stride_s; the row VALUES live on the device and are the caller's contract, as for the attention kernels' tables.
 * ARITHMETIC, NaN / Inf rule: vorta_expert_fidelity's, with x0 = ref and one error column (values widened exactly, one float32
 * rounding of the difference, float32 squares and sums, exact maxima; a NaN, or an Inf that meets an Inf, makes the sums AND the
 * maxima it reaches NaN, for that head only).
 * DETERMINISTIC: VORTA_SAMPLED_FIDELITY_PARTS partials per head slot over the fixed ranges of sample positions [b per, (b + 1)
 * per), per = ceil(n_rows / PARTS); a 16-lane quarter wave owns every 16th row of a range, 16 bytes a lane, the next row's
 * loads in flight; lanes meet by shuffles, the four waves through LDS, the partial goes to the workspace with plain vector
 * stores and a second launch joins a slot's parts as a fixed shuffle tree.  No float atomic; the same bits on every run and stream.
 * (16 parts: at n_rows = 2048 a head is 512 KiB a tensor -- 128 rows a workgroup, 8 visits a lane; 24 heads give 384 workgroups.)
 * LONGEST CHAIN of float32 roundings a sum passes through = VORTA_SAMPLED_FIDELITY_CHAIN(n_rows):
 *     2 (the rounded difference, squared) + 4 (a row's 8 squares: d^2, one fma, two tree levels) + V (one add per row a lane
 *     visits, V = ceil(per / 16)) + 6 (wave shuffles) + 2 (four waves) + 4 (16 parts) + 1 (the linear bound's slack, n <= 4096)
 * and every term is non-negative: |sum - exact| <= CHAIN 2^-24 exact.  n_rows = 2048: 27, i.e. 1.6e-6.  A row's sum takes
 * VORTA_SAMPLED_FIDELITY_ROW_CHAIN = 2 + 4 + 4 (the quarter wave's shuffles) + 1 roundings.
 * Error codes as for vorta_expert_fidelity: VORTA_EINVAL for a wrong struct_size, negative sizes, a null or misaligned output
 * (4 bytes), row table (4 bytes; null only with n_rows == 0), head list or device count (4 bytes) or workspace (16 bytes), a null
 * or misaligned tensor (16-byte aligned rows; null only with n_rows == 0); VORTA_EUNSUPPORTED for a dtype other than bf16 / fp16
 * or head_dim != 128.  Everything is looked at before anything is launched.  n_heads == 0 is VORTA_OK and launches nothing;
 * n_rows == 0 is VORTA_OK and writes zeros for the listed heads.
 */
#define VORTA_SAMPLED_FIDELITY_PARTS 16
#define VORTA_SAMPLED_FIDELITY_WS_FLOATS 8 /* per head slot and part */
#define VORTA_SAMPLED_FIDELITY_CHAIN(n_rows) \
  (((((int64_t)(n_rows) + VORTA_SAMPLED_FIDELITY_PARTS - 1) / VORTA_SAMPLED_FIDELITY_PARTS + 15) / 16) + 19)
#define VORTA_SAMPLED_FIDELITY_ROW_CHAIN 11
typedef struct vorta_sampled_fidelity_args {
  uint32_t struct_size; /* = sizeof(vorta_sampled_fidelity_args) = vorta_sampled_fidelity_args_size() */
  int32_t dtype, head_dim;
  int32_t n_heads;            /* head slots in this launch (upper bound when n_heads_dev is set) */
  int32_t n_rows;             /* the sample size n */
  int32_t reserved;
  vorta_tensor ref;           /* (H, n_rows, D): the dense reference rows, indexed by the head */
  vorta_tensor out;           /* (H, S[+T], D) view of the routed output, dtype of ref, read in place */
  const int32_t* rows;        /* [n_rows]: the physical row of `out` for sample position p */
  const int32_t* head_list;   /* [n_heads] or NULL */
  const int32_t* n_heads_dev; /* optional device count: slots >= *n_heads_dev write nothing */
  float* sq_ref;              /* out, indexed by the head */
  float* max_ref;             /* out, indexed by the head */
  float* sq_err;              /* out, indexed by the head */
  float* max_err;             /* out, indexed by the head */
  float* range_ref;           /* out, indexed by the head, or NULL */
  float* row_sq_err;          /* out [head][n_rows], or NULL */
  float* ws;                  /* workspace, n_heads * PARTS * WS_FLOATS floats, 16-byte aligned (caller-owned) */
} vorta_sampled_fidelity_args;

int vorta_sampled_fidelity(const vorta_sampled_fidelity_args* args, void* hip_stream);
int vorta_sampled_fidelity_args_size(void);

/*
 * vorta_gather_sample_rows (ABI 9, a pure addition: a binding asks for the symbol and for vorta_gather_sample_rows_args_size();
 * vorta_sizeof keeps its 17 indices) -- the glue of a PER-EXPERT fidelity measurement on sampled rows (what every expert would
 * have written at a sample of n_rows query rows; the reference has no such measurement).  One launch fills up to three compact
 * (H, n_rows, D) buffers, indexed by the HEAD, for head slot y < n_heads (< *n_heads_dev when given), head h = head_list ?
 * head_list[y] : y, and sample position p < n_rows:
 *     dst_q[h][p]    = q[h][rows[p]]                       the row's own query (dense attention, the sliding tile)
 *     dst_qrep[h][p] = q[h][rep(y, p)]                     the query that stands for the row under the coreset expert:
 *         rep(y, p) = rows[p], unless win[p] >= 0 and rows[p] is among drop_rows[y][win[p]][0 .. n_dup): then the centre of the
 *         window, keep_rows[y][win[p]] (vorta_coreset_select's lists: positions < G of a keep list are the centres, a dropped
 *         margin is written the centre's output).  win[p] = the coreset window of position p, -1 for a token outside the whole
 *         windows (partial geometry) or a text token; rows, keep_rows and drop_rows all hold PHYSICAL rows of q.
 *     dst_out[h][p]  = out[h][rows[p]]                     the routed output as launched
 * A destination with ptr NULL is not written (and its sources need not be given).  Heads the launch does not name, and slots
 * at or past *n_heads_dev, keep what the destinations held; nothing outside dst[h][0 .. n_rows)[0 .. 128) is written.  head_list
 * names distinct heads: every destination row has one writer; no atomics; the same bits on every run.  Row addresses are
 * 64-bit (head * stride_h + row * stride_s); a lane moves 16 bytes.  The row and window VALUES live on the device and are the
 * caller's contract, as for the attention kernels' tables.
 * VORTA_EINVAL for a wrong struct_size, negative sizes, more than 65535 head slots, a misaligned table, head list or device
 * count (4 bytes), a misaligned tensor (16-byte aligned rows), a wanted destination whose source or tables are null while
 * n_rows > 0; VORTA_EUNSUPPORTED for a dtype other than bf16 / fp16 or head_dim != 128.  Everything is looked at before
 * anything is launched.  n_heads == 0 and n_rows == 0 are VORTA_OK and launch nothing.
 */
typedef struct vorta_gather_sample_rows_args {
  uint32_t struct_size; /* = sizeof(vorta_gather_sample_rows_args) = vorta_gather_sample_rows_args_size() */
  int32_t dtype, head_dim;
  int32_t n_heads;            /* head slots in this launch (upper bound when n_heads_dev is set) */
  int32_t n_rows;             /* the sample size n */
  int32_t n_dup;              /* entries of one window's drop list: g - 1 - n_keep */
  vorta_tensor q;             /* (H, S[+T], D) view, read in place */
  vorta_tensor out;           /* (H, S[+T], D) view of the routed output, dtype of q; needed for dst_out only */
  vorta_tensor dst_q;         /* (H, n_rows, D), or ptr NULL */
  vorta_tensor dst_qrep;      /* (H, n_rows, D), or ptr NULL */
  vorta_tensor dst_out;       /* (H, n_rows, D), or ptr NULL */
  const int32_t* rows;        /* [n_rows]: the physical row of q / out for sample position p */
  const int32_t* win;         /* [n_rows]: the coreset window of position p, or -1; needed for dst_qrep only */
  const int32_t* keep_rows;   /* [slot][>= G]: vorta_coreset_select's keep list (its centres are read); dst_qrep only */
  int64_t keep_rows_stride_h;
  const int32_t* drop_rows;   /* [slot][G][n_dup]: its drop list; dst_qrep only */
  int64_t drop_rows_stride_h;
  const int32_t* head_list;   /* [n_heads] or NULL */
  const int32_t* n_heads_dev; /* optional device count: slots >= *n_heads_dev write nothing */
} vorta_gather_sample_rows_args;

int vorta_gather_sample_rows(const vorta_gather_sample_rows_args* args, void* hip_stream);
int vorta_gather_sample_rows_args_size(void);

/*
 * vorta_route_fidelity (ABI 9, a pure addition: a binding asks for the symbol and for vorta_route_fidelity_args_size();
 * vorta_sizeof keeps its 17 indices) -- head routing from MEASURED statistics, on the device: from the record of a per-expert
 * measurement (vorta_expert_fidelity's sq_ref / sq_err, e.g. on sampled rows) to the head -> expert table and the per-expert
 * head lists + counts, in vorta_route_scores' layout, so the expert launches take them without a host read.  The reference
 * has no counterpart (its routes come from a trained router).  One launch of one workgroup: launch latency.  No atomics; the
 * same bits on every run.  The rule is the host function's (vorta.patch.routes_from_fidelity), which is the definition.
 *
 * Relative error.  It follows ExpertFidelity.rel_error() exactly, in float32:
 *   - rel = sqrt(sq_err / sq_ref).
 *   - The division and the square root are correctly rounded.
 *   - sq_ref == 0 gives 0 where sq_err == 0, and +inf otherwise.
 *   - NaN stays NaN.
 *
 * Mode 0 (error bound).
 *   - Of the sparse experts whose rel <= (float)max_rel_error, take the one with the smaller work.
 *   - On equal work, take expert 2.
 *   - Where no sparse expert qualifies, take expert 0.
 *   - NaN meets no bound.
 *   - The host function compares a float32 tensor with a Python scalar.  That compares in float32, so the bound is a float.
 *
 * Mode 1 (FLOP budget).
 *   - A head's candidate is the sparse expert with the smaller rel.  Only experts with work[e] < work[0] and a finite rel
 *     count.  On equal rel, take the smaller work, then expert 2.
 *   - A head with no such expert has no candidate.
 *   - Heads are ranked by (rel of candidate, head id) ascending.
 *   - Start with every head on expert 0.
 *   - Walk the ranking.  While cost > max_flops_share * (heads * work[0]), move the next head to its candidate.
 *   - cost = n0*work[0] + n1*work[1] + n2*work[2], evaluated in double from the integer counts, left to right (every product
 *     and sum rounded on its own: no fused multiply-add).  The order of moves then cannot change its bits.
 *   - Stop when the cost is within the budget or the candidates run out.
 *   - max_flops_share >= 1 moves nothing.
 *
 * VORTA_EINVAL for a wrong struct_size; a null sq_ref, sq_err, expert_of_head, head_lists or head_counts; heads outside
 * 1..1024; a mode other than 0 or 1; in mode 0 a NaN or negative bound, in mode 1 a NaN or non-positive share; a work entry
 * that is not positive and finite.  Everything is looked at before anything is launched.
 */
typedef struct vorta_route_fidelity_args {
  uint32_t struct_size;      /* = sizeof(vorta_route_fidelity_args) = vorta_route_fidelity_args_size() */
  int32_t heads;             /* 1..1024 */
  const float* sq_ref;       /* [heads] */
  const float* sq_err;       /* [heads][3]; column 0 coreset, column 1 sliding tile (ExpertFidelity's layout); column 2 is not read */
  int32_t mode;              /* 0 = error bound, 1 = FLOP budget */
  float max_rel_error;       /* mode 0: >= 0 */
  double work[3];            /* FLOPs of one head under expert 0 / 1 / 2 (patch.fidelity.expert_work); all > 0 */
  double max_flops_share;    /* mode 1: > 0 */
  int32_t* expert_of_head;   /* [heads] */
  int32_t* head_lists;       /* [3][heads], ascending head ids; entries at or past the count are not written */
  int32_t* head_counts;      /* [3] */
  float* flops_share;        /* optional, 1 float: (n0 w0 + n1 w1 + n2 w2) / (heads w0), in double, rounded once */
} vorta_route_fidelity_args;

int vorta_route_fidelity(const vorta_route_fidelity_args* args, void* hip_stream);
int vorta_route_fidelity_args_size(void);

/*
 * vorta_route_fidelity_tiers (ABI 9, a pure addition: a binding asks for the symbol and for
 * vorta_route_fidelity_tiers_args_size(); vorta_sizeof keeps its 17 indices) -- vorta_route_fidelity's error-bound rule over
 * (precision tier, expert) PAIRS: the record holds, per tier the call may launch in, what each expert of each head writes IN
 * THAT TIER'S PRECISION against the one dense reference in the input dtype, so the bound covers the precision of what is
 * launched.  One launch of one workgroup; no atomics; the same bits on every run.  The rule is the host function's
 * (vorta.patch.routes_from_fidelity_tiers), which is the definition.
 *
 * Tiers are the CALLER'S, cheapest first, 1..3 of them; the kernel knows them by index only.
 *
 * Candidates.  A candidate is a pair (t, e): tier index t, expert e.
 *   - Its rel is vorta_route_fidelity's, in float32 from sq_err[t][h][c] and sq_ref[h]: c = 0 for expert 1 (coreset), c = 1
 *     for expert 2 (sliding tile), c = 2 for expert 0 (full attention in tier t).  Same zero rules; NaN meets no bound.
 *   - exact_tier names the tier whose full attention IS the reference: its column 2 is not read and counts as 0.  -1: none.
 *   - Its cost is work[e] * tier_cost[t] in double, one rounded product (no fused multiply-add).
 *
 * Rule.
 *   - Per head, take the cheapest candidate with rel <= (float)max_rel_error.
 *   - On equal cost, take the lower tier index, then the larger expert id.
 *   - Where no candidate qualifies, take full attention (expert 0) in the LAST tier.
 *
 * The FLOP-budget rule has no tier form: mode 1 is VORTA_EINVAL.
 *
 * VORTA_EINVAL for whatever vorta_route_fidelity refuses (a wrong struct_size; a null sq_ref, sq_err, expert_of_head,
 * head_lists or head_counts; heads outside 1..1024; a NaN or negative bound; a work entry that is not positive and finite),
 * and for a null tier_of_head, a mode other than 0, n_tiers outside 1..3, exact_tier outside -1..n_tiers-1 and a tier_cost
 * entry (of the first n_tiers) that is not positive and finite.  Everything is looked at before anything is launched.
 */
typedef struct vorta_route_fidelity_tiers_args {
  uint32_t struct_size;      /* = sizeof(vorta_route_fidelity_tiers_args) = vorta_route_fidelity_tiers_args_size() */
  int32_t heads;             /* 1..1024 */
  int32_t n_tiers;           /* 1..3 */
  int32_t exact_tier;        /* -1..n_tiers-1 */
  const float* sq_ref;       /* [heads] */
  const float* sq_err;       /* [n_tiers][heads][3]; column 0 coreset, column 1 sliding tile, column 2 full attention, in that tier */
  int32_t mode;              /* 0 = error bound; anything else: VORTA_EINVAL */
  float max_rel_error;       /* >= 0 */
  double work[3];            /* FLOPs of one head under expert 0 / 1 / 2 (patch.fidelity.expert_work); all > 0 */
  double tier_cost[3];       /* cost of a FLOP in tier t relative to any common unit; the first n_tiers > 0 */
  int32_t* expert_of_head;   /* [heads] */
  int32_t* tier_of_head;     /* [heads], the caller's tier index */
  int32_t* head_lists;       /* [n_tiers][3][heads], ascending head ids; entries at or past the count are not written */
  int32_t* head_counts;      /* [n_tiers][3] */
  float* cost_share;         /* optional, 1 float: sum over (t, e), t-major, of n[t][e] (work[e] tier_cost[t]), over
                                heads (work[0] tier_cost[n_tiers-1]), in double from the integer counts, rounded once */
} vorta_route_fidelity_tiers_args;

int vorta_route_fidelity_tiers(const vorta_route_fidelity_tiers_args* args, void* hip_stream);
int vorta_route_fidelity_tiers_args_size(void);

/*
 * vorta_route_budget_tiers (ABI 9, a pure addition: a binding asks for the symbol and for
 * vorta_route_budget_tiers_args_size(); vorta_sizeof keeps its 17 indices) -- routing over (precision tier, expert) PAIRS by
 * a COST budget: spend at most max_cost_share of what the layer costs with every head on full attention in the last tier,
 * on any expert in any tier, so that the largest per-head error is as small as that buys.  The record, the tiers, the
 * candidates, their rel and their cost are vorta_route_fidelity_tiers'.  One launch of one workgroup; no atomics; the same
 * bits on every run.  The rule is the host function's (vorta.patch.routes_within_cost_share), which is the definition.
 *
 * Definitions.
 *   - state(r), r >= 0 in float32: the table vorta_route_fidelity_tiers gives at max_rel_error = r.
 *   - cost(table): the sum over (t, e), t-major, of n[t][e] * (work[e] * tier_cost[t]) from the integer counts, in double,
 *     every product and sum rounded on its own; an empty list adds nothing.
 *   - budget = max_cost_share * (heads * (work[0] * tier_cost[n_tiers-1])), rounded products in that order.  A table is
 *     within the budget unless cost > budget: equality is within.
 *   - The levels are 0 and every finite rel of a candidate.
 *
 * Rule.
 *   - r* is the smallest level whose state is within the budget.  Where no level is, the candidates ran out: r* is the
 *     largest level, the result is state(r*), and cost_share > max_cost_share shows it.
 *   - r* == 0: the result is state(0).
 *   - Else start from state(r-), r- the largest level below r*.  The heads whose pair in state(r*) is STRICTLY cheaper than
 *     their pair in state(r-) move to it in ascending head id, one at a time, until the cost is within the budget.  No
 *     other head moves: an equal cost moves nothing.
 *   - level receives r*: every head that had a qualifying candidate is within it on the sampled rows.
 * The result minimises the largest per-head rel over all assignments within the budget.  With one tier this is NOT
 * vorta_route_fidelity's mode 1, which gives a head one candidate; here a head may step down twice.
 *
 * The kernel sorts nothing: 32 passes bisect the bit pattern of r*, 1 pass finds r-, 11 bisect the head index of the partial
 * step; every trip count is fixed at launch.  The two bisections (midpoint lo + (hi - lo) / 2 over 0 .. the pattern of +inf;
 * (lo + hi) / 2 over 0 .. heads) are how the host function finds r* and the partial step too.  They are the searches of the
 * rule wherever cost(state(r)) does not grow with r: always with an exact tier, and without one whenever full attention in the
 * last tier is the dearest pair.  In another order they still end on a level whose state is within the budget (or report that
 * the candidates ran out), but a smaller such level may exist.
 *
 * VORTA_EINVAL for whatever vorta_route_fidelity_tiers refuses (a wrong struct_size; a null sq_ref, sq_err, expert_of_head,
 * tier_of_head, head_lists or head_counts; heads outside 1..1024; n_tiers outside 1..3; exact_tier outside -1..n_tiers-1; a
 * work entry, or a tier_cost entry of the first n_tiers, that is not positive and finite), and for a max_cost_share that is
 * NaN, zero or negative.  Everything is looked at before anything is launched.
 */
typedef struct vorta_route_budget_tiers_args {
  uint32_t struct_size;      /* = sizeof(vorta_route_budget_tiers_args) = vorta_route_budget_tiers_args_size() */
  int32_t heads;             /* 1..1024 */
  int32_t n_tiers;           /* 1..3 */
  int32_t exact_tier;        /* -1..n_tiers-1 */
  const float* sq_ref;       /* [heads] */
  const float* sq_err;       /* [n_tiers][heads][3]; column 0 coreset, column 1 sliding tile, column 2 full attention, in that tier */
  double max_cost_share;     /* > 0 */
  double work[3];            /* FLOPs of one head under expert 0 / 1 / 2 (patch.fidelity.expert_work); all > 0 */
  double tier_cost[3];       /* cost of a FLOP in tier t relative to any common unit; the first n_tiers > 0 */
  int32_t* expert_of_head;   /* [heads] */
  int32_t* tier_of_head;     /* [heads], the caller's tier index */
  int32_t* head_lists;       /* [n_tiers][3][heads], ascending head ids; entries at or past the count are not written */
  int32_t* head_counts;      /* [n_tiers][3] */
  float* cost_share;         /* optional, 1 float: cost(result) over heads (work[0] tier_cost[n_tiers-1]), in double, rounded once */
  float* level;              /* optional, 1 float: r* */
} vorta_route_budget_tiers_args;

int vorta_route_budget_tiers(const vorta_route_budget_tiers_args* args, void* hip_stream);
int vorta_route_budget_tiers_args_size(void);

/*
 * vorta_route_repair (ABI 9, a pure addition: a binding asks for the symbol and for vorta_route_repair_args_size();
 * vorta_sizeof keeps its 17 indices) -- verify what a forward LAUNCHED against a stated error and repair the routes.  The
 * record is vorta_sampled_fidelity's (sq_ref, sq_err per head: the rows the routed launches wrote against dense attention in
 * the input dtype).  One launch of one workgroup; no atomics; the same bits on every run.  The rule is the host function's
 * (vorta.patch.repair_routes), which is the definition.
 *
 * Rule, per head h with e = expert_of_head[h] and t = tier_of_head[h] (0 where tier_of_head is NULL):
 *   - e == -1 (no list names the head), or (e, t) == (0, exact_tier) (its launch IS the reference): not checked, kept.
 *   - Otherwise rel = vorta_route_fidelity's, in float32 from sq_err[h] and sq_ref[h] (same zero rules).  rel <= repair_above:
 *     kept.  Else (NaN included: NaN meets no bound) repaired: the head becomes (expert 0, exact_tier).
 *
 * expert_of_head, tier_of_head, head_lists and head_counts are updated IN PLACE: they are the buffers the next launches read.
 * The lists are rebuilt from the head tables (the old lists are not read), ascending; entries at or past a count are not
 * written.  repair_list receives the heads repaired by THIS launch, ascending, repair_count their number: the head list and
 * device count of the dense launch that overwrites them.  The rule is idempotent: a second launch on the same record repairs
 * nothing.
 *
 * VORTA_EINVAL for a wrong struct_size; a null sq_ref, sq_err, expert_of_head, head_lists, head_counts, repair_list or
 * repair_count; a null tier_of_head with n_tiers > 1; heads outside 1..1024; n_tiers outside 1..3; exact_tier outside
 * 0..n_tiers-1; a NaN or negative bound.  Everything is looked at before anything is launched.
 */
typedef struct vorta_route_repair_args {
  uint32_t struct_size;      /* = sizeof(vorta_route_repair_args) = vorta_route_repair_args_size() */
  int32_t heads;             /* 1..1024 */
  int32_t n_tiers;           /* 1..3 */
  int32_t exact_tier;        /* 0..n_tiers-1: the tier whose full attention is the reference */
  float repair_above;        /* >= 0 */
  int32_t reserved;          /* 0 */
  const float* sq_ref;       /* [heads] */
  const float* sq_err;       /* [heads] */
  int32_t* expert_of_head;   /* [heads], in place: -1, 0, 1, 2 */
  int32_t* tier_of_head;     /* [heads], in place, the caller's tier index; may be NULL when n_tiers == 1 */
  int32_t* head_lists;       /* [n_tiers][3][heads], rewritten: ascending head ids; entries at or past the count are not written */
  int32_t* head_counts;      /* [n_tiers][3], rewritten */
  int32_t* repair_list;      /* [heads]: the heads repaired by this launch, ascending; entries at or past the count are not written */
  int32_t* repair_count;     /* [1] */
  int32_t* state_of_head;    /* optional, [heads]: 0 not checked, 1 kept, 2 repaired */
  float* rel;                /* optional, [heads]: the error as checked; NaN for a head that was not checked */
} vorta_route_repair_args;

int vorta_route_repair(const vorta_route_repair_args* args, void* hip_stream);
int vorta_route_repair_args_size(void);

/*
 * vorta_seq_row_map -- physical row of every token for the zero-copy Ulysses layout.
 * After all_to_all_single of a sequence-sharded (H, S/P, D) tensor (vorta/ulysses/utils.py:61-91) rank r
 * holds P chunks of (H/P, S/P, D); the reference re-packs them into (H/P, S, D) with two
 * transpose+contiguous passes (:84-89).  Instead the kernels read the received buffer in place:
 * token s of local head hl is row  (s / Sl) * (Hl*Sl) + hl*Sl + s % Sl  ->  row_map[s] holds the part
 * that does not depend on the head, the head term is stride_h = Sl rows.
 */
int vorta_seq_row_map(int32_t* row_map, int32_t n_tokens, int32_t seg_len, int32_t seg_stride_rows, void* hip_stream);

/*
 * vorta_permute_heads -- the staging passes of the Ulysses exchange in one launch (vorta/ulysses/utils.py:61-91 does
 * them as transpose + .contiguous() per tensor and direction; A13 in SURVEY.md §8a).  For up to four (heads, n_rows, D)
 * views at once:
 *     dst[t][dst_map ? dst_map[h] : h][r][:] = src[t][src_map ? src_map[h] : h][r][:]      h < heads, r < n_rows
 * Send side: q, k, v projection views -> head-ordered contiguous blocks (src_map = head order), and the replicated text
 * rows behind each local head slot; receive side: the head-ordered output back into the (rows, H*D) result (dst_map).
 * The maps are device arrays of `heads` entries; a map must not repeat a head on the destination side, and no source may
 * overlap a destination (the copy is not an in-place permutation).
 */
typedef struct vorta_permute_args {
  uint32_t struct_size;
  int32_t dtype, head_dim, heads, n_rows, n_tensors; /* dtype: VORTA_BF16 / VORTA_FP16 (2-byte) or VORTA_FP8E4M3 */
  vorta_tensor src[4];
  vorta_tensor dst[4];
  const int32_t* src_map; /* [heads] or NULL */
  const int32_t* dst_map; /* [heads] or NULL */
} vorta_permute_args;

int vorta_permute_heads(const vorta_permute_args* args, void* hip_stream);

/* Introspection */
int vorta_abi_version(void);
const char* vorta_build_info(void); /* static string: arch, compiler */
int vorta_last_hip_error(void);     /* last hipError_t seen by a failed launch in this thread */
int vorta_sizeof(int which);        /* 0 tensor, 1 attn_args, 2 coreset_args, 3 sta_args, 4 router_args, 5 norm_rope_args,
                                       6 mix_args, 7 fp8_quant_args, 8 attn_fp8_ext, 9 permute_args, 10 fp8_v_args,
                                       11 i8_quant_args, 12 attn_i8_ext, 13 attn_bwd_args, 14 mix_bwd_args, 15 cast_args,
                                       16 norm_rope_bwd_args (-1 from a library without vorta_qk_norm_rope_bwd) */

#ifdef __cplusplus
}
#endif
#endif /* VORTA_HIP_H */
