// The query rows a per-expert fidelity measurement on SAMPLED rows needs, gathered compactly, for gfx950:
// include/vorta_hip.h vorta_gather_sample_rows.
//
// One launch fills up to three (H, n, D) buffers for the head slots of a head list: the queries of the sampled rows
// (dst_q: what dense attention and the sliding tile read), the queries that REPRESENT them under the coreset expert
// (dst_qrep: the row itself, or the centre of its window when the head's selection dropped the row) and the rows of the
// routed output as launched (dst_out).  A 16-lane quarter wave per 256-byte row, 16 bytes a lane, two sample positions per
// quarter wave with all their loads requested before the first store; the drop-list scan (g - 1 - n_keep entries, 5 at the
// published geometries) is strided over the 16 lanes and joined by one ballot.  HBM / latency bound: n = 2048 and 24 heads
// are 48 Ki rows of 256 B per buffer.  Every destination row has one writer (a head is named once, a position belongs to one
// quarter wave); no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace {

constexpr int POS_PER_WG = 32;  // 16 quarter waves x 2 positions

struct GParams {
  const char* q; int64_t q_sh, q_ss;  // bytes
  const char* out; int64_t out_sh, out_ss;
  char* dst_q; int64_t dq_sh, dq_ss;
  char* dst_qrep; int64_t dr_sh, dr_ss;
  char* dst_out; int64_t do_sh, do_ss;
  const int32_t* rows;
  const int32_t* win;
  const int32_t* keep_rows; int64_t keep_sh;  // elements
  const int32_t* drop_rows; int64_t drop_sh;
  const int32_t* head_list;
  const int32_t* n_heads_dev;
  int n_rows, n_dup;
};

__global__ __launch_bounds__(256) void gather_sample_rows_kernel(const GParams p) {
  const int slot = blockIdx.y;
  if (p.n_heads_dev && slot >= *p.n_heads_dev) return;  // (uniform over the workgroup)
  const int head = p.head_list ? p.head_list[slot] : slot;
  const int sub = threadIdx.x & 15, quarter = threadIdx.x >> 4;
  const int lane_group = (threadIdx.x & 63) >> 4;  // the quarter's place in its wave: its 16 bits of a ballot
  const int64_t pos[2] = {(int64_t)blockIdx.x * POS_PER_WG + quarter, (int64_t)blockIdx.x * POS_PER_WG + 16 + quarter};
  bool live[2];
  int row[2], rep[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    live[i] = pos[i] < p.n_rows;
    row[i] = rep[i] = live[i] ? p.rows[pos[i]] : 0;
  }
  if (p.dst_qrep) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int w = live[i] ? p.win[pos[i]] : -1;
      bool hit = false;
      if (w >= 0) {
        const int32_t* d = p.drop_rows + (int64_t)slot * p.drop_sh + (int64_t)w * p.n_dup;
        for (int j = sub; j < p.n_dup; j += 16) hit |= d[j] == row[i];
      }
      // (every lane of the wave votes: a quarter without a live position votes no)
      const unsigned long long votes = __ballot(hit);
      if ((votes >> (16 * lane_group)) & 0xffffull) rep[i] = p.keep_rows[(int64_t)slot * p.keep_sh + w];
    }
  }
  const int64_t hq = (int64_t)head * p.q_sh + sub * 16;
  u32x4 vq[2] = {}, vr[2] = {}, vo[2] = {};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (!live[i]) continue;
    if (p.dst_q) vq[i] = *(const u32x4*)(p.q + hq + (int64_t)row[i] * p.q_ss);
    if (p.dst_qrep) vr[i] = *(const u32x4*)(p.q + hq + (int64_t)rep[i] * p.q_ss);
    if (p.dst_out) vo[i] = *(const u32x4*)(p.out + (int64_t)head * p.out_sh + (int64_t)row[i] * p.out_ss + sub * 16);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (!live[i]) continue;
    if (p.dst_q) *(u32x4*)(p.dst_q + (int64_t)head * p.dq_sh + pos[i] * p.dq_ss + sub * 16) = vq[i];
    if (p.dst_qrep) *(u32x4*)(p.dst_qrep + (int64_t)head * p.dr_sh + pos[i] * p.dr_ss + sub * 16) = vr[i];
    if (p.dst_out) *(u32x4*)(p.dst_out + (int64_t)head * p.do_sh + pos[i] * p.do_ss + sub * 16) = vo[i];
  }
}

// strides and alignment of a 16-bit (H, rows, 128) view moved 16 bytes a lane
bool rows16(const vorta_tensor& t) {
  return !((uintptr_t)t.ptr & 15) && t.stride_s % 8 == 0 && t.stride_h % 8 == 0;
}

bool words(const void* q) { return !((uintptr_t)q & 3); }

}  // namespace

extern "C" int vorta_gather_sample_rows_args_size(void) { return (int)sizeof(vorta_gather_sample_rows_args); }

extern "C" int vorta_gather_sample_rows(const vorta_gather_sample_rows_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_gather_sample_rows_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128) return VORTA_EUNSUPPORTED;
  if (a->n_heads < 0 || a->n_rows < 0 || a->n_dup < 0) return VORTA_EINVAL;
  if (a->n_heads > 65535) return VORTA_EINVAL;  // (one grid row per head slot)
  if (!words(a->rows) || !words(a->win) || !words(a->keep_rows) || !words(a->drop_rows) || !words(a->head_list) ||
      !words(a->n_heads_dev))
    return VORTA_EINVAL;
  if (!rows16(a->q) || !rows16(a->out) || !rows16(a->dst_q) || !rows16(a->dst_qrep) || !rows16(a->dst_out)) return VORTA_EINVAL;
  if (a->keep_rows_stride_h < 0 || a->drop_rows_stride_h < 0) return VORTA_EINVAL;
  const bool any_dst = a->dst_q.ptr || a->dst_qrep.ptr || a->dst_out.ptr;
  if (a->n_rows > 0 && any_dst) {
    if (!a->rows) return VORTA_EINVAL;
    if ((a->dst_q.ptr || a->dst_qrep.ptr) && !a->q.ptr) return VORTA_EINVAL;
    if (a->dst_out.ptr && !a->out.ptr) return VORTA_EINVAL;
    if (a->dst_qrep.ptr && (!a->win || !a->keep_rows || (a->n_dup > 0 && !a->drop_rows))) return VORTA_EINVAL;
  }
  if (a->n_heads == 0 || a->n_rows == 0 || !any_dst) return VORTA_OK;
  GParams p{};
  p.q = (const char*)a->q.ptr; p.q_sh = a->q.stride_h * 2; p.q_ss = a->q.stride_s * 2;
  p.out = (const char*)a->out.ptr; p.out_sh = a->out.stride_h * 2; p.out_ss = a->out.stride_s * 2;
  p.dst_q = (char*)a->dst_q.ptr; p.dq_sh = a->dst_q.stride_h * 2; p.dq_ss = a->dst_q.stride_s * 2;
  p.dst_qrep = (char*)a->dst_qrep.ptr; p.dr_sh = a->dst_qrep.stride_h * 2; p.dr_ss = a->dst_qrep.stride_s * 2;
  p.dst_out = (char*)a->dst_out.ptr; p.do_sh = a->dst_out.stride_h * 2; p.do_ss = a->dst_out.stride_s * 2;
  p.rows = a->rows; p.win = a->win;
  p.keep_rows = a->keep_rows; p.keep_sh = a->keep_rows_stride_h;
  p.drop_rows = a->drop_rows; p.drop_sh = a->drop_rows_stride_h;
  p.head_list = a->head_list; p.n_heads_dev = a->n_heads_dev;
  p.n_rows = a->n_rows; p.n_dup = a->n_dup;
  const dim3 grid((unsigned)((a->n_rows + POS_PER_WG - 1) / POS_PER_WG), (unsigned)a->n_heads);
  hipLaunchKernelGGL(gather_sample_rows_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
