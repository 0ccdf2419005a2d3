// Head routing over (precision tier, expert) pairs from measured per-head statistics for gfx950: include/vorta_hip.h
// vorta_route_fidelity_tiers.
//
// route_fidelity.hip's error-bound rule with one more axis: the record holds, per precision tier the call may launch in, what
// every expert of every head writes IN THAT PRECISION against the one dense reference, and ONE launch of ONE workgroup turns
// it into the head -> (tier, expert) tables and the per-(tier, expert) head lists + counts on the DEVICE, by the rule
// patch/fidelity.py routes_from_fidelity_tiers states on the host.  No atomics; the same bits on every run.
//
// Arithmetic the host rule fixes, and this file keeps:
//   * rel is route_fidelity.hip's (route_rel_error.h: float32, a correctly rounded divide and square root);
//   * the cost of a candidate is work[e] * tier_cost[t] in double, one rounded product; the cost share sums n[t][e] * cost
//     from the integer counts, t-major, every product and sum rounded on its own -- contraction is off for the whole file.
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
constexpr int MAX_TIERS = 3;
constexpr int THREADS = 256;

struct TParams {
  const float* sq_ref; const float* sq_err;
  int H, n_tiers, exact_tier;
  float bound;
  double cost[MAX_TIERS][3];  // work[e] * tier_cost[t], formed on the host side of the launch: the same one rounded product
  int32_t* expert; int32_t* tier; int32_t* lists; int32_t* counts; float* cost_share;
};

__global__ __launch_bounds__(THREADS) void route_fidelity_tiers_kernel(const TParams p) {
  __shared__ int s_pair[MAX_HEADS];  // tier * 3 + expert of every head
  const int tid = threadIdx.x;
  const int H = p.H, T = p.n_tiers;
  for (int h = tid; h < H; h += THREADS) {
    const float ref = p.sq_ref[h];
    int best = (T - 1) * 3;  // no candidate within the bound: full attention in the last tier
    double best_cost = 0.0;
    bool found = false;
    // tiers ascending, experts descending, a strictly smaller cost replaces: equal cost keeps the lower tier, then the larger expert
    for (int t = 0; t < T; ++t) {
      const float* err = p.sq_err + ((size_t)t * H + h) * 3;
      for (int e = 2; e >= 0; --e) {
        const float rel = (e == 0 && t == p.exact_tier) ? 0.f : vorta_route::rel_error(err[e == 0 ? 2 : e - 1], ref);
        if (!(rel <= p.bound)) continue;  // (NaN meets no bound)
        const double c = p.cost[t][e];
        if (!found || c < best_cost) {
          found = true;
          best_cost = c;
          best = t * 3 + e;
        }
      }
    }
    s_pair[h] = best;
    p.expert[h] = best % 3;
    p.tier[h] = best / 3;
  }
  __syncthreads();
  if (tid < T * 3) {  // one lane per (tier, expert) list, [n_tiers][3][heads]
    int n = 0;
    for (int h = 0; h < H; ++h)
      if (s_pair[h] == tid) p.lists[(size_t)tid * H + n++] = h;
    p.counts[tid] = n;
  }
  if (tid == 64 && p.cost_share) {  // (a wave of its own: the list lanes above are in wave 0)
    double sum = 0.0;
    for (int i = 0; i < T * 3; ++i) {
      int n = 0;
      for (int h = 0; h < H; ++h) n += s_pair[h] == i;
      if (n) sum = sum + (double)n * p.cost[i / 3][i % 3];  // (an empty list adds nothing, whatever its cost)
    }
    *p.cost_share = (float)(sum / ((double)H * p.cost[T - 1][0]));
  }
}

bool positive_finite(double x) { return x > 0.0 && x <= DBL_MAX; }  // (a NaN fails both)

}  // namespace

extern "C" int vorta_route_fidelity_tiers_args_size(void) { return (int)sizeof(vorta_route_fidelity_tiers_args); }

extern "C" int vorta_route_fidelity_tiers(const vorta_route_fidelity_tiers_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_route_fidelity_tiers_args)) return VORTA_EINVAL;
  if (a->heads < 1 || a->heads > MAX_HEADS) return VORTA_EINVAL;
  if (a->n_tiers < 1 || a->n_tiers > MAX_TIERS) return VORTA_EINVAL;
  if (a->exact_tier < -1 || a->exact_tier >= a->n_tiers) return VORTA_EINVAL;
  if (a->mode != 0) return VORTA_EINVAL;  // the FLOP budget has no tier form
  if (!a->sq_ref || !a->sq_err || !a->expert_of_head || !a->tier_of_head || !a->head_lists || !a->head_counts)
    return VORTA_EINVAL;
  if (!(a->max_rel_error >= 0.f)) return VORTA_EINVAL;  // (a NaN fails every comparison)
  for (int e = 0; e < 3; ++e)
    if (!positive_finite(a->work[e])) return VORTA_EINVAL;
  for (int t = 0; t < a->n_tiers; ++t)
    if (!positive_finite(a->tier_cost[t])) return VORTA_EINVAL;
  TParams p{};
  p.sq_ref = a->sq_ref; p.sq_err = a->sq_err;
  p.H = a->heads; p.n_tiers = a->n_tiers; p.exact_tier = a->exact_tier;
  p.bound = a->max_rel_error;
  for (int t = 0; t < a->n_tiers; ++t)
    for (int e = 0; e < 3; ++e) p.cost[t][e] = a->work[e] * a->tier_cost[t];
  p.expert = a->expert_of_head; p.tier = a->tier_of_head; p.lists = a->head_lists; p.counts = a->head_counts;
  p.cost_share = a->cost_share;
  hipLaunchKernelGGL(route_fidelity_tiers_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)hip_stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
