// Head routing from measured per-head statistics for gfx950: include/vorta_hip.h vorta_route_fidelity.
//
// Launch-latency work, like router.hip's kernels: ONE launch of ONE workgroup turns the (sq_ref, sq_err) record of a
// per-expert measurement (vorta_expert_fidelity's layout) into the head -> expert table and the per-expert head lists +
// counts on the DEVICE, in vorta_route_scores' layout, by the rule patch/fidelity.py routes_from_fidelity states on the
// host.  No atomics; the same bits on every run.
//
// Arithmetic the host rule fixes, and this file keeps:
//   * rel = sqrt(sq_err / sq_ref) in float32, both operations correctly rounded (no fast-math here: a head whose error
//     sits exactly on the bound must fall on the same side as on the host);
//   * the cost of a routing is evaluated in double FROM THE INTEGER COUNTS, (n0 w0 + n1 w1) + n2 w2, each product and each
//     sum rounded on its own -- contraction into fused multiply-adds is switched off for the whole file, since a fused
//     product would not be the host's bits.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "vorta_hip.h"
#include "common.h"
#include "route_rel_error.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_HEADS = 1024;
constexpr int THREADS = 256;

struct FParams {
  const float* sq_ref; const float* sq_err;
  int H, mode;
  float bound;
  double w0, w1, w2, share;
  int32_t* expert; int32_t* lists; int32_t* counts; float* flops_share;
};

using vorta_route::rel_error;  // ExpertFidelity.rel_error() of one (head, column); route_fidelity_tiers.hip forms the same

__device__ __forceinline__ double cost_of(int n0, int n1, int n2, const FParams& p) {
  return ((double)n0 * p.w0 + (double)n1 * p.w1) + (double)n2 * p.w2;
}

__global__ __launch_bounds__(THREADS) void route_fidelity_kernel(const FParams p) {
  __shared__ int s_expert[MAX_HEADS];   // the table; mode 1: a head's candidate until the walk moves it
  __shared__ float s_key[MAX_HEADS];    // mode 1: rel of the candidate
  __shared__ int s_order[MAX_HEADS];    // mode 1: rank -> head, -1 past the candidates
  const int tid = threadIdx.x;
  const int H = p.H;
  for (int h = tid; h < H; h += THREADS) {
    const float ref = p.sq_ref[h];
    const float r1 = rel_error(p.sq_err[h * 3 + 0], ref);
    const float r2 = rel_error(p.sq_err[h * 3 + 1], ref);
    int e = 0;
    if (p.mode == 0) {
      // the cheaper of the sparse experts within the bound (NaN meets none); equal work: expert 2
      const bool ok1 = r1 <= p.bound, ok2 = r2 <= p.bound;
      if (ok1 && ok2) e = p.w1 < p.w2 ? 1 : 2;
      else if (ok1) e = 1;
      else if (ok2) e = 2;
    } else {
      // the candidate: the sparse expert with the smaller rel among those cheaper than full attention with a finite rel;
      // equal rel: the smaller work, then expert 2
      const bool c1 = p.w1 < p.w0 && isfinite(r1), c2 = p.w2 < p.w0 && isfinite(r2);
      float key = 0.f;
      if (c1 && c2) e = r1 < r2 ? 1 : r2 < r1 ? 2 : p.w1 < p.w2 ? 1 : 2;
      else if (c1) e = 1;
      else if (c2) e = 2;
      if (e) key = e == 1 ? r1 : r2;
      s_key[h] = key;
      s_order[h] = -1;
    }
    s_expert[h] = e;
  }
  __syncthreads();
  if (p.mode == 1) {
    // rank sort of the candidates by (rel, head id): a head's rank is the number of candidates ahead of it
    for (int h = tid; h < H; h += THREADS) {
      if (!s_expert[h]) continue;
      const float key = s_key[h];
      int rank = 0;
      for (int j = 0; j < H; ++j)
        rank += (s_expert[j] != 0 && (s_key[j] < key || (s_key[j] == key && j < h))) ? 1 : 0;
      s_order[rank] = h;
    }
    __syncthreads();
    if (tid == 0) {
      // the walk, by one lane: every head on expert 0; while the cost is over the budget, the next head of the ranking moves
      const double budget = p.share * ((double)H * p.w0);
      int n0 = H, n1 = 0, n2 = 0, moved = 0;
      while (moved < H && s_order[moved] >= 0 && cost_of(n0, n1, n2, p) > budget) {
        const int e = s_expert[s_order[moved]];
        --n0;
        if (e == 1) ++n1; else ++n2;
        ++moved;
      }
      for (int i = moved; i < H && s_order[i] >= 0; ++i) s_expert[s_order[i]] = 0;  // the candidates that stay
    }
    __syncthreads();
  }
  for (int h = tid; h < H; h += THREADS) p.expert[h] = s_expert[h];
  if (tid < 3) {
    int n = 0;
    for (int h = 0; h < H; ++h)
      if (s_expert[h] == tid) p.lists[tid * H + n++] = h;
    p.counts[tid] = n;
  }
  if (tid == 64 && p.flops_share) {  // (a wave of its own: the three list lanes above are in wave 0)
    int n1 = 0, n2 = 0;
    for (int h = 0; h < H; ++h) {
      n1 += s_expert[h] == 1;
      n2 += s_expert[h] == 2;
    }
    *p.flops_share = (float)(cost_of(H - n1 - n2, n1, n2, p) / ((double)H * p.w0));
  }
}

bool positive_finite(double x) { return x > 0.0 && x <= DBL_MAX; }  // (a NaN fails both)

}  // namespace

extern "C" int vorta_route_fidelity_args_size(void) { return (int)sizeof(vorta_route_fidelity_args); }

extern "C" int vorta_route_fidelity(const vorta_route_fidelity_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_route_fidelity_args)) return VORTA_EINVAL;
  if (a->heads < 1 || a->heads > MAX_HEADS) return VORTA_EINVAL;
  if (a->mode != 0 && a->mode != 1) return VORTA_EINVAL;
  if (!a->sq_ref || !a->sq_err || !a->expert_of_head || !a->head_lists || !a->head_counts) return VORTA_EINVAL;
  if (a->mode == 0 && !(a->max_rel_error >= 0.f)) return VORTA_EINVAL;   // (a NaN fails every comparison)
  if (a->mode == 1 && !(a->max_flops_share > 0.0)) return VORTA_EINVAL;
  for (int e = 0; e < 3; ++e)
    if (!positive_finite(a->work[e])) return VORTA_EINVAL;
  FParams p{a->sq_ref, a->sq_err, a->heads, a->mode, a->max_rel_error, a->work[0], a->work[1], a->work[2],
            a->max_flops_share, a->expert_of_head, a->head_lists, a->head_counts, a->flops_share};
  hipLaunchKernelGGL(route_fidelity_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)hip_stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
