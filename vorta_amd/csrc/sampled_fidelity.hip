// Per-head fidelity of a ROUTED call's output against dense attention on a sample of query rows, for gfx950:
// include/vorta_hip.h vorta_sampled_fidelity.
//
// vorta_expert_fidelity's frame (csrc/expert_fidelity.hip) with two differences: the second operand is read IN PLACE through a
// row table (out[head][rows[p]], 64-bit row addresses: the routed output of a head is up to 30 MB, the sample 512 KiB), and the
// launch takes the attention kernels' head lists with their device counts, so that it follows a router's decision without a
// host read.  A 16-lane quarter wave per 256-byte row, 16-byte loads, the next row's loads (and the row id after that) in
// flight; VORTA_SAMPLED_FIDELITY_PARTS = 16 fixed ranges of sample positions per head slot -- at n = 2048 a workgroup reads 128
// rows of each tensor, 8 visits a lane, and a layer of 24 measured heads is 384 workgroups: latency-bound, so neither one
// workgroup a head nor the 64 parts of the full-size kernel (32 rows each, more time in the joins than in the rows).  Every
// partial a fixed tree, a second launch for the parts.  No float atomics: the same bits on every run.
//
// LONGEST CHAIN of fp32 roundings a sum passes through (VORTA_SAMPLED_FIDELITY_CHAIN(n_rows) of the header; the tests derive
// their bound from it): 2 for the rounded difference, squared; 4 for a row's eight squares (d^2, one fma, two tree levels); V =
// ceil(ceil(n_rows / PARTS) / 16) adds into the lane's running sum; 6 wave shuffles; 2 for the four waves; 4 for the 16 parts; 1
// of slack that makes the linear bound rigorous: V + 19.  A row's own sum (row_sq_err): 2 + 4 + 4 quarter-wave shuffles + 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace {

constexpr int PARTS = VORTA_SAMPLED_FIDELITY_PARTS;
constexpr int WSF = VORTA_SAMPLED_FIDELITY_WS_FLOATS;
// a partial: 0 sum x0^2 | 1 sum d^2 | 2 max |d| | 3 max x0 | 4 min x0
constexpr int NV = 5;

struct SParams {
  const char* ref; int64_t ref_sh, ref_ss;  // bytes
  const char* out; int64_t out_sh, out_ss;
  const int32_t* rows;
  const int32_t* head_list;
  const int32_t* n_heads_dev;
  float* ws;  // [slots][PARTS][WSF]
  float *sq_ref, *max_ref, *sq_err, *max_err, *range_ref, *row_sq_err;
  int n_rows;
};

// eight squares as a fixed tree: (d0^2 + d1^2) ... by one product and one fma, then two levels of adds
__device__ inline float sq_tree(const float (&d)[8]) {
  const float q0 = __builtin_fmaf(d[1], d[1], d[0] * d[0]), q1 = __builtin_fmaf(d[3], d[3], d[2] * d[2]);
  const float q2 = __builtin_fmaf(d[5], d[5], d[4] * d[4]), q3 = __builtin_fmaf(d[7], d[7], d[6] * d[6]);
  return (q0 + q1) + (q2 + q3);
}

__device__ inline float combine(int v, float a, float b) {  // how value v of a partial meets another: sum, max or min
  return v < 2 ? a + b : (v < 4 ? fmaxf(a, b) : fminf(a, b));
}

template <typename T, bool ROWS>
__global__ __launch_bounds__(256) void sampled_fidelity_partial_kernel(const SParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  __shared__ float red[4][NV];
  const int slot = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
  if (p.n_heads_dev && slot >= *p.n_heads_dev) return;  // (uniform over the workgroup)
  const int head = p.head_list ? p.head_list[slot] : slot;
  const int per = (p.n_rows + PARTS - 1) / PARTS;
  const int r0 = (int)min((int64_t)part * per, (int64_t)p.n_rows), r1 = (int)min((int64_t)r0 + per, (int64_t)p.n_rows);
  const int sub = threadIdx.x & 15;
  const char* bref = p.ref + (int64_t)head * p.ref_sh + sub * 16;
  const char* bout = p.out + (int64_t)head * p.out_sh + sub * 16;
  float* rowsum = ROWS ? p.row_sq_err + (int64_t)head * p.n_rows : nullptr;
  float val[NV] = {0.f, 0.f, 0.f, -INFINITY, INFINITY};
  int64_t pos = r0 + (threadIdx.x >> 4);  // (64-bit: pos + 32 is formed next to n_rows)
  V8 a0 = {}, a1 = {};
  int id_next = 0;  // the physical row of position pos + 16
  if (pos < r1) {
    a0 = *(const V8*)(bref + pos * p.ref_ss);
    a1 = *(const V8*)(bout + (int64_t)p.rows[pos] * p.out_ss);
    if (pos + 16 < r1) id_next = p.rows[pos + 16];
  }
  while (pos < r1) {
    // the next row's loads, and the row id of the one after, are in flight while this row is reduced
    const int64_t nx = pos + 16;
    V8 n0 = a0, n1 = a1;
    int id_after = 0;
    if (nx < r1) {
      n0 = *(const V8*)(bref + nx * p.ref_ss);
      n1 = *(const V8*)(bout + (int64_t)id_next * p.out_ss);
      if (nx + 16 < r1) id_after = p.rows[nx + 16];
    }
    float f0[8], d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f0[i] = (float)a0[i];
      val[3] = fmaxf(val[3], f0[i]);
      val[4] = fminf(val[4], f0[i]);
    }
    val[0] += sq_tree(f0);
#pragma unroll
    for (int i = 0; i < 8; ++i) { d[i] = (float)a1[i] - f0[i]; val[2] = fmaxf(val[2], fabsf(d[i])); }
    const float s = sq_tree(d);
    val[1] += s;
    if (ROWS) {
      float r = s;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) r += __shfl_xor(r, m);
      if (sub == 0) rowsum[pos] = r;
    }
    a0 = n0; a1 = n1;
    id_next = id_after;
    pos = nx;
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) val[v] = combine(v, val[v], __shfl_xor(val[v], m));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][v] = val[v];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int v = threadIdx.x;
    p.ws[((int64_t)slot * PARTS + part) * WSF + v] = combine(v, combine(v, red[0][v], red[1][v]), combine(v, red[2][v], red[3][v]));
  }
}

// one wave per head slot: lane b < 16 holds part b (the other lanes the neutral element), the parts meet in a shuffle tree.
// fmaxf / fminf drop a NaN, a sum keeps it, and a sum of squares is NaN exactly when one of its terms is: the maxima are NaN then.
__global__ __launch_bounds__(64) void sampled_fidelity_final_kernel(const SParams p) {
  const int slot = blockIdx.x;
  if (p.n_heads_dev && slot >= *p.n_heads_dev) return;
  const int head = p.head_list ? p.head_list[slot] : slot;
  static_assert(PARTS == 16 && WSF >= NV && WSF % 4 == 0, "one lane per part, float4 reads");
  float val[NV] = {0.f, 0.f, 0.f, -INFINITY, INFINITY};
  if (threadIdx.x < PARTS) {
    const float* w = p.ws + ((int64_t)slot * PARTS + threadIdx.x) * WSF;
    const f32x4 lo = *(const f32x4*)w;
    val[0] = lo[0]; val[1] = lo[1]; val[2] = lo[2]; val[3] = lo[3]; val[4] = w[4];
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int m = 1; m < PARTS; m <<= 1) val[v] = combine(v, val[v], __shfl_xor(val[v], m));
  }
  if (threadIdx.x != 0) return;
  const bool any = p.n_rows > 0, ref_nan = val[0] != val[0];
  p.sq_ref[head] = val[0];
  p.max_ref[head] = !any ? 0.f : (ref_nan ? val[0] : fmaxf(val[3], -val[4]));
  if (p.range_ref) p.range_ref[head] = !any ? 0.f : (ref_nan ? val[0] : val[3] - val[4]);
  p.sq_err[head] = val[1];
  p.max_err[head] = val[1] != val[1] ? val[1] : val[2];
}

// strides and alignment of a 16-bit (H, rows, 128) view read 16 bytes a lane; a null pointer passes only with no rows to read
bool rows16(const vorta_tensor& t, bool may_be_null) {
  if (!t.ptr && !may_be_null) return false;
  return !((uintptr_t)t.ptr & 15) && t.stride_s % 8 == 0 && t.stride_h % 8 == 0;
}

bool words(const void* q, bool required) { return q ? !((uintptr_t)q & 3) : !required; }

}  // namespace

extern "C" int vorta_sampled_fidelity_args_size(void) { return (int)sizeof(vorta_sampled_fidelity_args); }

extern "C" int vorta_sampled_fidelity(const vorta_sampled_fidelity_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_sampled_fidelity_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128) return VORTA_EUNSUPPORTED;
  if (a->n_heads < 0 || a->n_rows < 0) return VORTA_EINVAL;
  if (!words(a->sq_ref, true) || !words(a->max_ref, true) || !words(a->sq_err, true) || !words(a->max_err, true) ||
      !words(a->range_ref, false) || !words(a->row_sq_err, false))
    return VORTA_EINVAL;
  if (!words(a->rows, a->n_rows > 0) || !words(a->head_list, false) || !words(a->n_heads_dev, false)) return VORTA_EINVAL;
  if (!a->ws || ((uintptr_t)a->ws & 15)) return VORTA_EINVAL;
  if ((int64_t)a->n_heads * PARTS > 0x7fffffff) return VORTA_EINVAL;
  if (!rows16(a->ref, a->n_rows == 0) || !rows16(a->out, a->n_rows == 0)) return VORTA_EINVAL;
  if (a->n_heads == 0) return VORTA_OK;
  SParams p{};
  p.ref = (const char*)a->ref.ptr; p.ref_sh = a->ref.stride_h * 2; p.ref_ss = a->ref.stride_s * 2;
  p.out = (const char*)a->out.ptr; p.out_sh = a->out.stride_h * 2; p.out_ss = a->out.stride_s * 2;
  p.rows = a->rows; p.head_list = a->head_list; p.n_heads_dev = a->n_heads_dev;
  p.ws = a->ws; p.sq_ref = a->sq_ref; p.max_ref = a->max_ref; p.sq_err = a->sq_err; p.max_err = a->max_err;
  p.range_ref = a->range_ref; p.row_sq_err = a->row_sq_err; p.n_rows = a->n_rows;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)(a->n_heads * PARTS));
  // (n_rows == 0: every range is empty, nothing is read, the partials are the empty sums and the results are zeros)
  if (a->dtype == VORTA_BF16) {
    if (p.row_sq_err) hipLaunchKernelGGL((sampled_fidelity_partial_kernel<__bf16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((sampled_fidelity_partial_kernel<__bf16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (p.row_sq_err) hipLaunchKernelGGL((sampled_fidelity_partial_kernel<_Float16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((sampled_fidelity_partial_kernel<_Float16, false>), grid, dim3(256), 0, st, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vorta_set_hip_error(e);
  hipLaunchKernelGGL(sampled_fidelity_final_kernel, dim3((unsigned)a->n_heads), dim3(64), 0, st, p);
  e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
