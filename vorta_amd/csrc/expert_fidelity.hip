// Per-head fidelity of the sparse experts and of the mixed output against the full expert, for gfx950:
// include/vorta_hip.h vorta_expert_fidelity.
//
// The training-time forward holds the three experts' outputs of every head (routed.soft_mixture_attention); the torch
// expression for one error, (b1 - b0).float().square().sum(...), makes several fp32 temporaries of the buffers' size and about
// a dozen passes.  Here: one pass, four reads (three without `mixed`) and no large write, HBM-bound like vorta_mix_experts_bwd,
// whose frame this is -- a 16-lane quarter wave per 256-byte row, VORTA_FIDELITY_PARTS fixed row ranges per head, every
// partial a fixed tree, a second launch for the parts.  No float atomics: the same bits on every run.
//
// LONGEST CHAIN of fp32 roundings a sum passes through (VORTA_FIDELITY_CHAIN(n_rows) of the header; the tests derive their bound
// from it): 2 for the rounded difference, squared; 4 for a row's eight squares (d^2, one fma, two tree levels); V = ceil(ceil(
// n_rows / PARTS) / 16) adds into the lane's running sum; 6 wave shuffles; 2 for the four waves; 6 for the 64 parts; 1 of slack
// that makes the linear bound rigorous: V + 21.  All terms are non-negative, so the relative error is at most CHAIN 2^-24.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace {

constexpr int PARTS = VORTA_FIDELITY_PARTS;
constexpr int WSF = VORTA_FIDELITY_WS_FLOATS;
// a partial: 0 sum x0^2 | 1..3 sum d_j^2 | 4..6 max |d_j| | 7 max x0 | 8 min x0
constexpr int NV = 9;

struct FParams {
  const char* x[3]; int64_t x_sh[3], x_ss[3];  // bytes
  const char* m; int64_t m_sh, m_ss;
  float* ws;  // [heads][PARTS][WSF]
  float *sq_ref, *max_ref, *sq_err, *max_err, *range_ref;
  int heads, n_rows, has_mixed;
};

// eight squares as a fixed tree: (d0^2 + d1^2) ... by one product and one fma, then two levels of adds
__device__ inline float sq_tree(const float (&d)[8]) {
  const float q0 = __builtin_fmaf(d[1], d[1], d[0] * d[0]), q1 = __builtin_fmaf(d[3], d[3], d[2] * d[2]);
  const float q2 = __builtin_fmaf(d[5], d[5], d[4] * d[4]), q3 = __builtin_fmaf(d[7], d[7], d[6] * d[6]);
  return (q0 + q1) + (q2 + q3);
}

__device__ inline float combine(int v, float a, float b) {  // how value v of a partial meets another: sum, max or min
  return v < 4 ? a + b : (v < 8 ? fmaxf(a, b) : fminf(a, b));
}

template <typename T, bool MIX>
__global__ __launch_bounds__(256) void fidelity_partial_kernel(const FParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  __shared__ float red[4][NV];
  const int head = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
  const int64_t per = ((int64_t)p.n_rows + PARTS - 1) / PARTS;
  const int64_t r0 = part * per, r1 = min(r0 + per, (int64_t)p.n_rows);
  const int sub = threadIdx.x & 15;
  const char* b0 = p.x[0] + (int64_t)head * p.x_sh[0] + sub * 16;
  const char* b1 = p.x[1] + (int64_t)head * p.x_sh[1] + sub * 16;
  const char* b2 = p.x[2] + (int64_t)head * p.x_sh[2] + sub * 16;
  const char* b3 = MIX ? p.m + (int64_t)head * p.m_sh + sub * 16 : nullptr;
  float val[NV] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -INFINITY, INFINITY};
  int64_t row = r0 + (threadIdx.x >> 4);
  V8 a0 = {}, a1 = {}, a2 = {}, a3 = {};
  if (row < r1) {
    a0 = *(const V8*)(b0 + row * p.x_ss[0]); a1 = *(const V8*)(b1 + row * p.x_ss[1]); a2 = *(const V8*)(b2 + row * p.x_ss[2]);
    if (MIX) a3 = *(const V8*)(b3 + row * p.m_ss);
  }
  while (row < r1) {
    // the next row's loads are in flight while this row is reduced
    const int64_t nx = row + 16;
    V8 n0 = a0, n1 = a1, n2 = a2, n3 = a3;
    if (nx < r1) {
      n0 = *(const V8*)(b0 + nx * p.x_ss[0]); n1 = *(const V8*)(b1 + nx * p.x_ss[1]); n2 = *(const V8*)(b2 + nx * p.x_ss[2]);
      if (MIX) n3 = *(const V8*)(b3 + nx * p.m_ss);
    }
    float f0[8], d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f0[i] = (float)a0[i];
      val[7] = fmaxf(val[7], f0[i]);
      val[8] = fminf(val[8], f0[i]);
    }
    val[0] += sq_tree(f0);
#pragma unroll
    for (int i = 0; i < 8; ++i) { d[i] = (float)a1[i] - f0[i]; val[4] = fmaxf(val[4], fabsf(d[i])); }
    val[1] += sq_tree(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) { d[i] = (float)a2[i] - f0[i]; val[5] = fmaxf(val[5], fabsf(d[i])); }
    val[2] += sq_tree(d);
    if (MIX) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { d[i] = (float)a3[i] - f0[i]; val[6] = fmaxf(val[6], fabsf(d[i])); }
      val[3] += sq_tree(d);
    }
    a0 = n0; a1 = n1; a2 = n2; a3 = n3;
    row = nx;
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
    p.ws[((int64_t)head * PARTS + part) * WSF + v] = combine(v, combine(v, red[0][v], red[1][v]), combine(v, red[2][v], red[3][v]));
  }
}

// one wave per head: lane b holds part b, the 64 parts meet in a shuffle tree.  fmaxf / fminf drop a NaN, a sum keeps it, and a
// sum of squares is NaN exactly when one of its differences is: the maxima of such a column are NaN too.
__global__ __launch_bounds__(64) void fidelity_final_kernel(const FParams p) {
  const int head = blockIdx.x;
  static_assert(PARTS == 64, "one lane per part");
  const float* w = p.ws + ((int64_t)head * PARTS + threadIdx.x) * WSF;
  const f32x4 lo = *(const f32x4*)w, hi = *(const f32x4*)(w + 4);
  float val[NV] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3], w[8]};
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) val[v] = combine(v, val[v], __shfl_xor(val[v], m));
  }
  if (threadIdx.x != 0) return;
  const bool any = p.n_rows > 0, ref_nan = val[0] != val[0];
  p.sq_ref[head] = val[0];
  p.max_ref[head] = !any ? 0.f : (ref_nan ? val[0] : fmaxf(val[7], -val[8]));
  if (p.range_ref) p.range_ref[head] = !any ? 0.f : (ref_nan ? val[0] : val[7] - val[8]);
  const int cols = p.has_mixed ? 3 : 2;
  for (int j = 0; j < cols; ++j) {
    const float s = val[1 + j];
    p.sq_err[head * 3 + j] = s;
    p.max_err[head * 3 + j] = s != s ? s : val[4 + j];
  }
}

// strides and alignment of a 16-bit (H, n_rows, 128) view read 16 bytes a lane; a null pointer passes only with no rows to read
bool rows16(const vorta_tensor& t, bool may_be_null) {
  if (!t.ptr && !may_be_null) return false;
  return !((uintptr_t)t.ptr & 15) && t.stride_s % 8 == 0 && t.stride_h % 8 == 0;
}

bool floats(const float* q, bool required) { return q ? !((uintptr_t)q & 3) : !required; }

}  // namespace

extern "C" int vorta_fidelity_args_size(void) { return (int)sizeof(vorta_fidelity_args); }

extern "C" int vorta_expert_fidelity(const vorta_fidelity_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_fidelity_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128) return VORTA_EUNSUPPORTED;
  if (a->heads < 0 || a->n_rows < 0) return VORTA_EINVAL;
  if (!floats(a->sq_ref, true) || !floats(a->max_ref, true) || !floats(a->sq_err, true) || !floats(a->max_err, true) ||
      !floats(a->range_ref, false))
    return VORTA_EINVAL;
  if (!a->ws || ((uintptr_t)a->ws & 15)) return VORTA_EINVAL;
  if ((int64_t)a->heads * PARTS > 0x7fffffff) return VORTA_EINVAL;
  FParams p{};
  for (int e = 0; e < 3; ++e) {
    if (!rows16(a->x[e], a->n_rows == 0)) return VORTA_EINVAL;
    p.x[e] = (const char*)a->x[e].ptr; p.x_sh[e] = a->x[e].stride_h * 2; p.x_ss[e] = a->x[e].stride_s * 2;
  }
  p.has_mixed = a->mixed.ptr != nullptr;
  if (p.has_mixed) {
    if (!rows16(a->mixed, false)) return VORTA_EINVAL;
    p.m = (const char*)a->mixed.ptr; p.m_sh = a->mixed.stride_h * 2; p.m_ss = a->mixed.stride_s * 2;
  }
  if (a->heads == 0) return VORTA_OK;
  p.ws = a->ws; p.sq_ref = a->sq_ref; p.max_ref = a->max_ref; p.sq_err = a->sq_err; p.max_err = a->max_err;
  p.range_ref = a->range_ref; p.heads = a->heads; p.n_rows = a->n_rows;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)(a->heads * PARTS));
  // (n_rows == 0: every range is empty, nothing is read, the partials are the empty sums and the results are zeros)
  if (a->dtype == VORTA_BF16) {
    if (p.has_mixed) hipLaunchKernelGGL((fidelity_partial_kernel<__bf16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((fidelity_partial_kernel<__bf16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (p.has_mixed) hipLaunchKernelGGL((fidelity_partial_kernel<_Float16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((fidelity_partial_kernel<_Float16, false>), grid, dim3(256), 0, st, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vorta_set_hip_error(e);
  hipLaunchKernelGGL(fidelity_final_kernel, dim3((unsigned)a->heads), dim3(64), 0, st, p);
  e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
