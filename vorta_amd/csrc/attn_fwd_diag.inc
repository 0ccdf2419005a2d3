// Diagnostic build of the 16-bit attention loop (attn_fwd.hip includes this ahead of its kernels): -DVORTA_TRACE (suffixed
// libraries only: vorta_amd/build.py refuses extra flags for the product library; tools/trace_barrier.py reads the result)
// stamps the end-of-step wait and the barrier of attn_pipe_dma_body and leaves, per wave, the cycles of the loop, of its
// waits and of its barriers, the 100 MHz wall clock beside them and the hardware ids in ws_ml of an unsplit launch; the fused
// kernel adds a stamp at every workgroup's end (TRACE_WG_END_ below; tools/trace_fused_grid.py reads it).
// Results stay correct.  Without the flag every macro here is empty and the product library holds none of this.
#ifdef VORTA_TRACE
#define TRACE_ENTRY_() const long long tr_e0_ = wall_clock64();  /* workgroup entry, absolute (100 MHz) */
#define TRACE_VARS_()                                                             \
  long long tr_wait_ = 0, tr_bar_ = 0;                                            \
  const long long tr_t0_ = clock64();                                             \
  const long long tr_w0_ = wall_clock64();  /* constant 100 MHz: the shader clock over the loop follows from the two */
#define STEP_SYNC()                                                               \
  {                                                                               \
    const long long a_ = clock64();                                               \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                   \
    const long long b_ = clock64();                                               \
    asm volatile("s_barrier" ::: "memory");                                       \
    const long long c_ = clock64();                                               \
    tr_wait_ += b_ - a_;                                                          \
    tr_bar_ += c_ - b_;                                                           \
  }
#define TRACE_FLUSH_()                                                            \
  if (p.n_splits == 1 && p.ws_ml && lane == 0) {                                  \
    long long* tr = (long long*)p.ws_ml + ((int64_t)wg * NW + wave) * 8;          \
    tr[0] = clock64() - tr_t0_; tr[1] = tr_wait_; tr[2] = tr_bar_; tr[3] = blk1 - blk0; \
    tr[4] = wall_clock64() - tr_w0_;                                              \
    tr[5] = tr_e0_; tr[6] = wall_clock64();  /* absolute entry / end-of-loop times */ \
    tr[7] = (long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |   /* HW_ID */ \
            ((long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32);  /* XCC_ID */ \
  }
// end of a workgroup of the fused grid (attn_fwd_multi_kernel, behind the body: every exit of the body comes through here).
// Per wave, behind the records above ([workgroups][8 waves][8]): [workgroups][8 waves][2] = the 100 MHz wall clock once
// the wave's output stores have left, and the hardware ids (tools/trace_fused_grid.py)
#define TRACE_WG_END_(p_, wg_)                                                    \
  if ((p_).n_splits == 1 && (p_).ws_ml && (threadIdx.x & 63) == 0) {              \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                              \
    long long* te_ = (long long*)(p_).ws_ml + (int64_t)(p_).n_heads * (p_).wg_per_slot * 64 + \
                     ((int64_t)(wg_) * 8 + (threadIdx.x >> 6)) * 2;               \
    te_[0] = wall_clock64();                                                      \
    te_[1] = (long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |   /* HW_ID */ \
             ((long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32);  /* XCC_ID */ \
  }
#else
#define TRACE_ENTRY_()
#define TRACE_VARS_()
#define TRACE_FLUSH_()
#define TRACE_WG_END_(p_, wg_)
#endif
