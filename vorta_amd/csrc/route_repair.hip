// Verification of launched routes against a stated error, and their repair, for gfx950: include/vorta_hip.h vorta_route_repair.
//
// The routing kernels (route_fidelity.hip, route_fidelity_tiers.hip) bound what the CANDIDATE launches of a measuring forward
// write.  This one reads the record of what a forward DID launch (vorta_sampled_fidelity: sq_ref, sq_err per head), picks the
// heads that are over the bound, and rewrites the head -> (tier, expert) tables and the per-(tier, expert) head lists + counts
// IN PLACE so that those heads run full attention in the exact tier from now on -- the buffers the next forward's launches and
// a captured graph read -- and emits the list of heads repaired by this launch, which a dense launch takes as its head list.
// ONE launch of ONE workgroup; no atomics; the same bits on every run.  The rule is patch/fidelity.py repair_routes.
//
//   * rel is the routing kernels' (route_rel_error.h: float32, a correctly rounded divide and square root);
//   * the old lists are not read: the lists are rebuilt from the head tables, so a list entry at or past its count is
//     neither read nor written.
#include <hip/hip_runtime.h>
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
constexpr int NO_LIST = 15;   // the pair of a head no list names: no list lane has this index
constexpr int REPAIRED = 16;  // flag beside the pair: repaired by this launch

struct RParams {
  const float* sq_ref; const float* sq_err;
  int H, n_tiers, exact_tier;
  float bound;
  int32_t* expert; int32_t* tier; int32_t* lists; int32_t* counts;
  int32_t* repair_list; int32_t* repair_count; int32_t* state; float* rel;
};

__global__ __launch_bounds__(THREADS) void route_repair_kernel(const RParams p) {
  __shared__ int s_pair[MAX_HEADS];  // (tier * 3 + expert, or NO_LIST) | REPAIRED of every head, after the rule
  const int tid = threadIdx.x;
  const int H = p.H, T = p.n_tiers;
  for (int h = tid; h < H; h += THREADS) {
    const int e = p.expert[h];
    const int t = p.tier ? p.tier[h] : 0;
    int pair = NO_LIST, state = 0;
    float rel = NAN;
    if (e >= 0 && e < 3 && t >= 0 && t < T) {
      pair = t * 3 + e;
      if (!(e == 0 && t == p.exact_tier)) {
        rel = vorta_route::rel_error(p.sq_err[h], p.sq_ref[h]);
        if (rel <= p.bound) {  // (NaN meets no bound)
          state = 1;
        } else {
          state = 2;
          pair = (p.exact_tier * 3) | REPAIRED;
          p.expert[h] = 0;
          if (p.tier) p.tier[h] = p.exact_tier;
        }
      }
    }
    s_pair[h] = pair;
    if (p.state) p.state[h] = state;
    if (p.rel) p.rel[h] = rel;
  }
  __syncthreads();
  if (tid < T * 3) {  // one lane per (tier, expert) list, [n_tiers][3][heads]
    int n = 0;
    for (int h = 0; h < H; ++h)
      if ((s_pair[h] & (REPAIRED - 1)) == tid) p.lists[(size_t)tid * H + n++] = h;
    p.counts[tid] = n;
  }
  if (tid == 64) {  // (a wave of its own: the list lanes above are in wave 0)
    int n = 0;
    for (int h = 0; h < H; ++h)
      if (s_pair[h] & REPAIRED) p.repair_list[n++] = h;
    *p.repair_count = n;
  }
}

}  // namespace

extern "C" int vorta_route_repair_args_size(void) { return (int)sizeof(vorta_route_repair_args); }

extern "C" int vorta_route_repair(const vorta_route_repair_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_route_repair_args)) return VORTA_EINVAL;
  if (a->heads < 1 || a->heads > MAX_HEADS) return VORTA_EINVAL;
  if (a->n_tiers < 1 || a->n_tiers > MAX_TIERS) return VORTA_EINVAL;
  if (a->exact_tier < 0 || a->exact_tier >= a->n_tiers) return VORTA_EINVAL;
  if (!a->sq_ref || !a->sq_err || !a->expert_of_head || !a->head_lists || !a->head_counts || !a->repair_list ||
      !a->repair_count)
    return VORTA_EINVAL;
  if (!a->tier_of_head && a->n_tiers != 1) return VORTA_EINVAL;
  if (!(a->repair_above >= 0.f)) return VORTA_EINVAL;  // (a NaN fails every comparison)
  RParams p{};
  p.sq_ref = a->sq_ref; p.sq_err = a->sq_err;
  p.H = a->heads; p.n_tiers = a->n_tiers; p.exact_tier = a->exact_tier;
  p.bound = a->repair_above;
  p.expert = a->expert_of_head; p.tier = a->tier_of_head; p.lists = a->head_lists; p.counts = a->head_counts;
  p.repair_list = a->repair_list; p.repair_count = a->repair_count; p.state = a->state_of_head; p.rel = a->rel;
  hipLaunchKernelGGL(route_repair_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)hip_stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
