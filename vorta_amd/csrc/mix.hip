// Score-weighted sum of the three experts' outputs for gfx950: include/vorta_hip.h vorta_mix_experts.
//
// The training-time forward of the reference runs every head through all three experts and mixes the results
// (`_combine_attn_outputs`, hunyuan.py:509-513, wan.py:296-300: stack to (B,H,3,S,D), multiply by the scores,
// sum over the expert axis -- two more full-size temporaries).  Here: one pass, three reads + one write per
// element, fp32 accumulation, one rounding.  HBM-bound (4 x rows x 256 B per head); a 16-lane quarter wave
// per 256-byte row.  The backward pieces that are not attention live here too: vorta_mix_experts_bwd and vorta_cast_grads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace {

struct MParams {
  const char* x[3]; int64_t x_sh[3], x_ss[3];  // bytes
  char* o; int64_t o_sh, o_ss;
  const void* scores;  // [heads][3] in the I/O dtype (batch item 0)
  int heads, n_rows;
};

template <typename T>
__global__ __launch_bounds__(256) void mix_experts_kernel(const MParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  const int64_t item = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  if (item >= (int64_t)p.heads * p.n_rows) return;
  const int head = (int)(item / p.n_rows);
  const int64_t row = item - (int64_t)head * p.n_rows;
  const T* sc = (const T*)p.scores + head * 3;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float w = (float)sc[e];
    const V8 xv = *(const V8*)(p.x[e] + (int64_t)head * p.x_sh[e] + row * p.x_ss[e] + sub * 16);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += w * (float)xv[i];
  }
  V8 ov;
#pragma unroll
  for (int i = 0; i < 8; ++i) ov[i] = (T)acc[i];
  *(V8*)(p.o + (int64_t)head * p.o_sh + row * p.o_ss + sub * 16) = ov;
}

// ---- backward (vorta_mix_experts_bwd): dscores[h][e] = <d_out[h], x[e][h]> ----
// Part `b` of VORTA_MIX_BWD_PARTS owns a fixed range of the head's rows: every thread walks its rows in a fixed order, the
// 256 partials meet in a fixed shuffle / LDS tree and the second kernel adds the parts in order: no float atomics, the same
// bits on every run.
struct MBParams {
  const char* x[3]; int64_t x_sh[3], x_ss[3];  // bytes
  const char* g; int64_t g_sh, g_ss;
  float* ws;       // [heads][PARTS][4]
  float* dscores;  // [heads][3]
  int heads, n_rows;
};

template <typename T>
__global__ __launch_bounds__(256) void mix_bwd_partial_kernel(const MBParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  __shared__ float red[4][3];
  const int head = blockIdx.x / VORTA_MIX_BWD_PARTS, part = blockIdx.x % VORTA_MIX_BWD_PARTS;
  const int per = (p.n_rows + VORTA_MIX_BWD_PARTS - 1) / VORTA_MIX_BWD_PARTS;
  const int r0 = part * per, r1 = min(r0 + per, p.n_rows);
  const int sub = threadIdx.x & 15;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int row = r0 + (threadIdx.x >> 4); row < r1; row += 16) {
    const V8 gv = *(const V8*)(p.g + (int64_t)head * p.g_sh + (int64_t)row * p.g_ss + sub * 16);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const V8 xv = *(const V8*)(p.x[e] + (int64_t)head * p.x_sh[e] + (int64_t)row * p.x_ss[e] + sub * 16);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[e] += (float)gv[i] * (float)xv[i];
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc[e] += __shfl_xor(acc[e], m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][e] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < 3)
    p.ws[((int64_t)head * VORTA_MIX_BWD_PARTS + part) * 4 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(64) void mix_bwd_final_kernel(const MBParams p) {
  const int head = blockIdx.x, e = threadIdx.x;
  if (e >= 3) return;
  float s = 0.f;
  for (int b = 0; b < VORTA_MIX_BWD_PARTS; ++b) s += p.ws[((int64_t)head * VORTA_MIX_BWD_PARTS + b) * 4 + e];
  p.dscores[head * 3 + e] = s;
}

// ---- vorta_cast_grads: fp32 accumulation buffers -> 16-bit views, one rounding (to nearest even) ----
struct CParams {
  const float* src[3]; int64_t s_sh[3], s_ss[3];  // floats
  char* dst[3]; int64_t d_sh[3], d_ss[3];          // bytes
  int heads, n_rows, n_tensors;
};

template <typename T>
__global__ __launch_bounds__(256) void cast_grads_kernel(const CParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  const int64_t item = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const int64_t per = (int64_t)p.heads * p.n_rows;
  if (item >= per * p.n_tensors) return;
  const int t = (int)(item / per);
  const int64_t rem = item - t * per;
  const int head = (int)(rem / p.n_rows);
  const int64_t row = rem - (int64_t)head * p.n_rows;
  const float* sp;
  char* dp;
  // (selected, not indexed: a dynamic index into the by-value parameter block would go through scratch)
  if (t == 0) { sp = p.src[0] + head * p.s_sh[0] + row * p.s_ss[0]; dp = p.dst[0] + head * p.d_sh[0] + row * p.d_ss[0]; }
  else if (t == 1) { sp = p.src[1] + head * p.s_sh[1] + row * p.s_ss[1]; dp = p.dst[1] + head * p.d_sh[1] + row * p.d_ss[1]; }
  else { sp = p.src[2] + head * p.s_sh[2] + row * p.s_ss[2]; dp = p.dst[2] + head * p.d_sh[2] + row * p.d_ss[2]; }
  const f32x4 a = *(const f32x4*)(sp + sub * 8), b = *(const f32x4*)(sp + sub * 8 + 4);
  V8 ov;
#pragma unroll
  for (int i = 0; i < 4; ++i) { ov[i] = (T)a[i]; ov[4 + i] = (T)b[i]; }
  *(V8*)(dp + sub * 16) = ov;
}

bool rows16(const vorta_tensor& t, int elems_per_16b) {
  return t.ptr && !((uintptr_t)t.ptr & 15) && t.stride_s % elems_per_16b == 0 && t.stride_h % elems_per_16b == 0;
}

}  // namespace

extern "C" int vorta_mix_experts_bwd(const vorta_mix_bwd_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_mix_bwd_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128 || a->n_experts != 3) return VORTA_EUNSUPPORTED;
  if (a->heads <= 0 || a->n_rows < 0 || !a->dscores || !a->ws) return VORTA_EINVAL;
  if ((int64_t)a->heads * VORTA_MIX_BWD_PARTS > 0x7fffffff) return VORTA_EINVAL;
  MBParams p;
  for (int e = 0; e < 3; ++e) {
    if (!rows16(a->x[e], 8)) return VORTA_EINVAL;
    p.x[e] = (const char*)a->x[e].ptr; p.x_sh[e] = a->x[e].stride_h * 2; p.x_ss[e] = a->x[e].stride_s * 2;
  }
  if (!rows16(a->d_out, 8)) return VORTA_EINVAL;
  p.g = (const char*)a->d_out.ptr; p.g_sh = a->d_out.stride_h * 2; p.g_ss = a->d_out.stride_s * 2;
  p.ws = a->ws; p.dscores = a->dscores; p.heads = a->heads; p.n_rows = a->n_rows;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)(a->heads * VORTA_MIX_BWD_PARTS));
  if (a->dtype == VORTA_BF16) hipLaunchKernelGGL(mix_bwd_partial_kernel<__bf16>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(mix_bwd_partial_kernel<_Float16>, grid, dim3(256), 0, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vorta_set_hip_error(e);
  hipLaunchKernelGGL(mix_bwd_final_kernel, dim3((unsigned)a->heads), dim3(64), 0, st, p);
  e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

extern "C" int vorta_cast_grads(const vorta_cast_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_cast_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128) return VORTA_EUNSUPPORTED;
  if (a->heads <= 0 || a->n_rows < 0 || a->n_tensors < 1 || a->n_tensors > 3) return VORTA_EINVAL;
  CParams p{};
  for (int t = 0; t < a->n_tensors; ++t) {
    if (!rows16(a->src[t], 4) || !rows16(a->dst[t], 8)) return VORTA_EINVAL;
    p.src[t] = (const float*)a->src[t].ptr; p.s_sh[t] = a->src[t].stride_h; p.s_ss[t] = a->src[t].stride_s;
    p.dst[t] = (char*)a->dst[t].ptr; p.d_sh[t] = a->dst[t].stride_h * 2; p.d_ss[t] = a->dst[t].stride_s * 2;
  }
  if (a->n_rows == 0) return VORTA_OK;
  p.heads = a->heads; p.n_rows = a->n_rows; p.n_tensors = a->n_tensors;
  const int64_t items = (int64_t)p.heads * p.n_rows * p.n_tensors;
  if (items > 0x7fffffff0ll) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((items + 15) / 16));
  if (a->dtype == VORTA_BF16) hipLaunchKernelGGL(cast_grads_kernel<__bf16>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(cast_grads_kernel<_Float16>, grid, dim3(256), 0, st, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

extern "C" int vorta_mix_experts(const vorta_mix_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_mix_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128 || a->n_experts != 3) return VORTA_EUNSUPPORTED;
  if (a->heads <= 0 || a->n_rows < 0 || !a->scores || !a->out.ptr) return VORTA_EINVAL;
  if (a->n_rows == 0) return VORTA_OK;
  MParams p;
  for (int e = 0; e < 3; ++e) {
    const vorta_tensor& t = a->x[e];
    if (!t.ptr || ((uintptr_t)t.ptr & 15) || (t.stride_s % 8) || (t.stride_h % 8)) return VORTA_EINVAL;
    p.x[e] = (const char*)t.ptr; p.x_sh[e] = t.stride_h * 2; p.x_ss[e] = t.stride_s * 2;
  }
  if (((uintptr_t)a->out.ptr & 15) || (a->out.stride_s % 8) || (a->out.stride_h % 8)) return VORTA_EINVAL;
  p.o = (char*)a->out.ptr; p.o_sh = a->out.stride_h * 2; p.o_ss = a->out.stride_s * 2;
  p.scores = a->scores; p.heads = a->heads; p.n_rows = a->n_rows;
  const int64_t items = (int64_t)p.heads * p.n_rows;
  if (items > 0x7fffffff0ll) return VORTA_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((items + 15) / 16));
  if (a->dtype == VORTA_BF16) hipLaunchKernelGGL(mix_experts_kernel<__bf16>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(mix_experts_kernel<_Float16>, grid, dim3(256), 0, st, p);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
