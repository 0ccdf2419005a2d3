// Backward of the fused q/k RMSNorm + rotary embedding for gfx950: include/vorta_hip.h vorta_qk_norm_rope_bwd.
//
// The last kernel between dq / dk of the attention backward and the projections.  With the forward of csrc/qk_norm_rope.hip,
//   y = x * r * w,  r = rsqrt(mean(x^2) + eps)       out = interleaved-pair rotation of y by (cos, sin)
// and g = d(out), all in fp32:
//   dy[2i]   = g[2i] * cos[2i]     + g[2i+1] * sin[2i+1]
//   dy[2i+1] = g[2i+1] * cos[2i+1] - g[2i]   * sin[2i]               (rows >= rope_tokens, or no table: dy = g)
//   dx       = r * (w * dy) - x * r^3 / n * sum_n(w * dy * x)         (n = D, or H*D across heads; w = 1 without a weight)
//   dw[c]    = sum over rows of dy[c] * x[c] * r
// HBM-bound: x and g are read once, dx is written once (3 x rows x D x 2 B per tensor).  The forward's mapping is kept: a
// 16-lane quarter wave per 256-byte row (per-head form), a wave per token with the token held in registers in 16 bits
// (across-heads form); cos / sin are read once per token.  Unlike the forward, a workgroup walks several tokens (a grid of
// at most VORTA_NORM_ROPE_BWD_PARTS workgroups): each keeps its share of dw in registers, reduces it in a fixed order to ONE
// fp32 partial per channel in `ws` (plain vector stores) and a second kernel adds the partials in order -- no float atomics,
// the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"

namespace {

struct BParams {
  const char* x; int64_t x_sh, x_ss;  // bytes; the forward's INPUT
  const char* g; int64_t g_sh, g_ss;  // gradient of the forward's output
  char* dx; int64_t d_sh, d_ss;       // may alias g: a lane reads its 16 bytes of g before it writes the same 16 bytes of dx
  const void* w;                      // [D] (per head) or [H*D] (across heads), dtype of x; may be NULL
  const float* cs; const float* sn;   // [n_tokens][D] fp32 or NULL
  float* ws;                          // [gridDim.x][channels] partial sums of dw (DW instantiations)
  int heads, n_tokens, token_offset, rope_tokens;
  float eps;
};

__device__ __forceinline__ float q16_sum(float v) {
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

__device__ __forceinline__ void load_table(const float* t, int64_t token, int sub, float (&o)[8]) {
  const float* s = t + token * 128 + sub * 8;
  const f32x4 a = *(const f32x4*)s, b = *(const f32x4*)(s + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}

// g -> dy: the transpose of the forward's rotation (cos[2i], cos[2i+1], sin[2i], sin[2i+1] are four independent entries)
template <typename V8>
__device__ __forceinline__ void unrotate(const V8& gv, bool rot, const float (&cc)[8], const float (&sn)[8], float (&dy)[8]) {
  if (rot) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float g0 = (float)gv[2 * i], g1 = (float)gv[2 * i + 1];
      dy[2 * i] = g0 * cc[2 * i] + g1 * sn[2 * i + 1];
      dy[2 * i + 1] = g1 * cc[2 * i + 1] - g0 * sn[2 * i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) dy[i] = (float)gv[i];
  }
}

// per-head normalisation (HunyuanVideo): wave `w` of a workgroup owns token 4 b + w of every round, its four quarter waves
// every fourth head of it; UNR rows of x and of g in flight per quarter wave before the first is touched.
template <typename T, bool DW>
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_head_kernel(const BParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  constexpr int UNR = 6;
  __shared__ float red[DW ? 4 : 1][128];
  const int sub = threadIdx.x & 15;
  const int wave = threadIdx.x >> 6;
  const int hq = (threadIdx.x >> 4) & 3;
  float wf[8];
  if (p.w) {
    const V8 wv = *(const V8*)((const char*)p.w + sub * 16);
#pragma unroll
    for (int i = 0; i < 8; ++i) wf[i] = (float)wv[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) wf[i] = 1.f;
  }
  float dwa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int token = blockIdx.x * 4 + wave; token < p.n_tokens; token += gridDim.x * 4) {
    const bool rot = p.cs && token < p.rope_tokens;
    float cc[8], sn[8];
    if (rot) {
      load_table(p.cs, token, sub, cc);
      load_table(p.sn, token, sub, sn);
    }
    const int64_t row = (int64_t)p.token_offset + token;
    const char* xb = p.x + row * p.x_ss + sub * 16;
    const char* gb = p.g + row * p.g_ss + sub * 16;
    char* db = p.dx + row * p.d_ss + sub * 16;
    for (int h0 = hq; h0 < p.heads; h0 += 4 * UNR) {
      V8 xv[UNR], gv[UNR];
#pragma unroll
      for (int j = 0; j < UNR; ++j)
        if (h0 + 4 * j < p.heads) {
          xv[j] = *(const V8*)(xb + (int64_t)(h0 + 4 * j) * p.x_sh);
          gv[j] = *(const V8*)(gb + (int64_t)(h0 + 4 * j) * p.g_sh);
        }
#pragma unroll
      for (int j = 0; j < UNR; ++j) {
        if (h0 + 4 * j >= p.heads) break;
        float x[8], dy[8], ss = 0.f, dot = 0.f;
        unrotate(gv[j], rot, cc, sn, dy);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          x[i] = (float)xv[j][i];
          ss += x[i] * x[i];
          dot += wf[i] * dy[i] * x[i];
        }
        ss = q16_sum(ss);
        dot = q16_sum(dot);
        const float r = rsqrtf(ss * (1.f / 128.f) + p.eps);
        const float coef = r * r * r * (1.f / 128.f) * dot;
        V8 ov;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          ov[i] = (T)(r * (wf[i] * dy[i]) - x[i] * coef);
          if constexpr (DW) dwa[i] += dy[i] * x[i] * r;
        }
        *(V8*)(db + (int64_t)(h0 + 4 * j) * p.d_sh) = ov;
      }
    }
  }
  if constexpr (DW) {  // quarter waves of a wave, then the four waves, in a fixed order
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      dwa[i] += __shfl_xor(dwa[i], 16);
      dwa[i] += __shfl_xor(dwa[i], 32);
    }
    if ((threadIdx.x & 63) < 16) {
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][sub * 8 + i] = dwa[i];
    }
    __syncthreads();
    if (threadIdx.x < 128)
      p.ws[(int64_t)blockIdx.x * 128 + threadIdx.x] =
          (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// normalisation across all heads of a token (Wan): one wave per token, x and g kept in registers in 16 bits between the
// pass that takes the two sums (x^2 and w dy x: neither needs r) and the pass that writes dx
template <typename T, int MAXIT, bool DW>
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_token_kernel(const BParams p) {
  typedef __attribute__((ext_vector_type(8))) T V8;
  __shared__ float red[DW ? MAXIT * 512 : 4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int chunks = p.heads * 16;  // 16-byte chunks per token; chunk c = it * 64 + lane is channels 8 c .. 8 c + 7
  const float inv_n = 1.f / (float)(p.heads * 128);
  float dwa[DW ? MAXIT : 1][8];
  if constexpr (DW) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it)
#pragma unroll
      for (int i = 0; i < 8; ++i) dwa[it][i] = 0.f;
  }
  for (int token = blockIdx.x * 4 + wave; token < p.n_tokens; token += gridDim.x * 4) {
    const bool rot = p.cs && token < p.rope_tokens;
    float cc[8], sn[8];
    if (rot) {
      load_table(p.cs, token, lane & 15, cc);
      load_table(p.sn, token, lane & 15, sn);
    }
    const int64_t row = (int64_t)p.token_offset + token;
    V8 xv[MAXIT], gv[MAXIT];
    float ss = 0.f, dot = 0.f;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int c = it * 64 + lane;
      if (c < chunks) {
        const int head = c >> 4, sub = c & 15;
        xv[it] = *(const V8*)(p.x + (int64_t)head * p.x_sh + row * p.x_ss + sub * 16);
        gv[it] = *(const V8*)(p.g + (int64_t)head * p.g_sh + row * p.g_ss + sub * 16);
      }
    }
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int c = it * 64 + lane;
      if (c < chunks) {
        float dy[8];
        unrotate(gv[it], rot, cc, sn, dy);
        if (p.w) {
          const V8 wv = *(const V8*)((const char*)p.w + (int64_t)c * 16);
#pragma unroll
          for (int i = 0; i < 8; ++i) dy[i] *= (float)wv[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float f = (float)xv[it][i];
          ss += f * f;
          dot += dy[i] * f;
        }
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      ss += __shfl_xor(ss, s);
      dot += __shfl_xor(dot, s);
    }
    const float r = rsqrtf(ss * inv_n + p.eps);
    const float coef = r * r * r * inv_n * dot;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int c = it * 64 + lane;
      if (c < chunks) {
        const int head = c >> 4, sub = c & 15;
        float dy[8], wf[8];
        unrotate(gv[it], rot, cc, sn, dy);
        if (p.w) {
          const V8 wv = *(const V8*)((const char*)p.w + (int64_t)c * 16);
#pragma unroll
          for (int i = 0; i < 8; ++i) wf[i] = (float)wv[i];
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) wf[i] = 1.f;
        }
        V8 ov;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float f = (float)xv[it][i];
          ov[i] = (T)(r * (wf[i] * dy[i]) - f * coef);
          if constexpr (DW) dwa[it][i] += dy[i] * f * r;
        }
        *(V8*)(p.dx + (int64_t)head * p.d_sh + row * p.d_ss + sub * 16) = ov;
      }
    }
  }
  if constexpr (DW) {  // wave 0 stores its sums, waves 1, 2, 3 add theirs in turn: a fixed order
    for (int w = 0; w < 4; ++w) {
      if (wave == w) {
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const int c = it * 64 + lane;
          if (c < chunks) {
            f32x4* dst = (f32x4*)(red + c * 8);
            f32x4 a = {dwa[it][0], dwa[it][1], dwa[it][2], dwa[it][3]};
            f32x4 b = {dwa[it][4], dwa[it][5], dwa[it][6], dwa[it][7]};
            if (w) { a += dst[0]; b += dst[1]; }
            dst[0] = a;
            dst[1] = b;
          }
        }
      }
      __syncthreads();
    }
    f32x4* out = (f32x4*)(p.ws + (int64_t)blockIdx.x * chunks * 8);
    for (int j = threadIdx.x; j < chunks * 2; j += 256) out[j] = ((const f32x4*)red)[j];
  }
}

// dweight[c] = the partials of channel c added in workgroup order
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_final_kernel(const float* ws, float* dw, int parts, int channels) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= channels) return;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < parts; ++b) s += ws[(int64_t)b * channels + c];
  dw[c] = s;
}

template <typename T, bool DW>
int launch(const BParams& p, int across_heads, unsigned parts, hipStream_t st) {
  if (!across_heads) {
    hipLaunchKernelGGL((qk_norm_rope_bwd_head_kernel<T, DW>), dim3(parts), dim3(256), 0, st, p);
  } else {
    const int its = (p.heads * 16 + 63) / 64;
    if (its <= 3) hipLaunchKernelGGL((qk_norm_rope_bwd_token_kernel<T, 3, DW>), dim3(parts), dim3(256), 0, st, p);
    else if (its <= 6) hipLaunchKernelGGL((qk_norm_rope_bwd_token_kernel<T, 6, DW>), dim3(parts), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((qk_norm_rope_bwd_token_kernel<T, 10, DW>), dim3(parts), dim3(256), 0, st, p);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}

bool rows16(const vorta_tensor& t) {
  return t.ptr && !((uintptr_t)t.ptr & 15) && t.stride_s % 8 == 0 && t.stride_h % 8 == 0;
}

}  // namespace

extern "C" int vorta_qk_norm_rope_bwd(const vorta_norm_rope_bwd_args* b, void* hip_stream) {
  if (!b || b->struct_size != sizeof(vorta_norm_rope_bwd_args)) return VORTA_EINVAL;
  const vorta_norm_rope_args* a = &b->fwd;
  if (a->struct_size != sizeof(vorta_norm_rope_args)) return VORTA_EINVAL;
  if (a->dtype != VORTA_BF16 && a->dtype != VORTA_FP16) return VORTA_EUNSUPPORTED;
  if (a->head_dim != 128) return VORTA_EUNSUPPORTED;
  if (a->heads <= 0 || a->n_tokens < 0 || a->token_offset < 0 || a->rope_tokens < 0) return VORTA_EINVAL;
  if (a->across_heads && (a->heads * 16 + 63) / 64 > 10) return VORTA_EUNSUPPORTED;
  const int64_t channels = a->across_heads ? (int64_t)a->heads * 128 : 128;
  hipStream_t st = (hipStream_t)hip_stream;
  if (a->n_tokens == 0) {
    if (!b->dweight) return VORTA_OK;
    const hipError_t e = hipMemsetAsync(b->dweight, 0, (size_t)channels * sizeof(float), st);
    return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
  }
  if (!rows16(a->x) || !rows16(b->g) || !rows16(b->dx)) return VORTA_EINVAL;
  if ((a->cos == nullptr) != (a->sin == nullptr)) return VORTA_EINVAL;
  if (a->cos && (((uintptr_t)a->cos & 15) || ((uintptr_t)a->sin & 15))) return VORTA_EINVAL;
  if (a->weight && ((uintptr_t)a->weight & 15)) return VORTA_EINVAL;
  if ((int64_t)a->n_tokens * a->heads > 0x7fffffff0ll) return VORTA_EINVAL;
  const int64_t groups = ((int64_t)a->n_tokens + 3) / 4;
  const unsigned parts = (unsigned)(groups < VORTA_NORM_ROPE_BWD_PARTS ? groups : VORTA_NORM_ROPE_BWD_PARTS);
  if (b->dweight) {
    if (((uintptr_t)b->dweight & 3) || !b->ws || ((uintptr_t)b->ws & 15)) return VORTA_EINVAL;
    if (b->ws_floats < (int64_t)parts * channels) return VORTA_EINVAL;
  }
  BParams p{(const char*)a->x.ptr, a->x.stride_h * 2, a->x.stride_s * 2,
            (const char*)b->g.ptr, b->g.stride_h * 2, b->g.stride_s * 2,
            (char*)b->dx.ptr, b->dx.stride_h * 2, b->dx.stride_s * 2,
            a->weight, a->cos, a->sin, b->dweight ? b->ws : nullptr,
            a->heads, a->n_tokens, a->token_offset, a->rope_tokens, a->eps};
  int rc;
  if (a->dtype == VORTA_BF16) rc = b->dweight ? launch<__bf16, true>(p, a->across_heads, parts, st) : launch<__bf16, false>(p, a->across_heads, parts, st);
  else rc = b->dweight ? launch<_Float16, true>(p, a->across_heads, parts, st) : launch<_Float16, false>(p, a->across_heads, parts, st);
  if (rc != VORTA_OK || !b->dweight) return rc;
  hipLaunchKernelGGL(qk_norm_rope_bwd_final_kernel, dim3((unsigned)((channels + 255) / 256)), dim3(256), 0, st, b->ws, b->dweight,
                     (int)parts, (int)channels);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
