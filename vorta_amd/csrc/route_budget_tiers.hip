// Head routing over (precision tier, expert) pairs by a COST BUDGET from measured per-head statistics for gfx950:
// include/vorta_hip.h vorta_route_budget_tiers.
//
// route_fidelity_tiers.hip answers "the cheapest pair within this error"; this file answers "the smallest error this cost
// buys": spend at most max_cost_share of the layer with every head on full attention in the last tier, over any expert in any
// tier, so that the largest per-head error is as small as the budget allows.  ONE launch of ONE workgroup turns the record
// into the head -> (tier, expert) tables, the per-(tier, expert) head lists + counts, the cost share and the level (the error
// the budget bought) on the DEVICE, by the rule patch/fidelity.py routes_within_cost_share states on the host.  No atomics;
// the same bits on every run.
//
// Scheme.  state(r) = route_fidelity_tiers.hip's table at bound r; cost(state(r)) does not grow with r, and non-negative
// float32 values order like their bit patterns.  So nothing is sorted:
//   1. 32 passes bisect the bit pattern of r for r*, the smallest r whose state is within the budget (31 halve the range
//      0 .. the pattern of +inf, which stands for "no level is"; the 32nd leaves the trip count a round constant).  Per pass
//      every lane finds its heads' pairs in at most nine compares and an integer count reduction gives the cost.
//   2. 1 pass takes two integer maxima over the finite rel: the largest level below r* (r-), and the largest level.
//   3. 11 passes bisect the head index m of the partial step: heads below m whose pair at r* is strictly cheaper than their
//      pair at r- move to it, the others keep state(r-)'s.  The cost does not grow with m.
// 32 + 1 + 11 passes, every trip count fixed at launch; no spin-wait, no data-dependent while.  A cost is formed from integer
// counts by every lane alike, so the moves cannot change its bits.
//
// Arithmetic the host rule fixes, and this file keeps:
//   * rel is route_fidelity.hip's (route_rel_error.h: float32, a correctly rounded divide and square root);
//   * the cost of a candidate is work[e] * tier_cost[t] in double, one rounded product; a table's cost sums n[t][e] * cost
//     from the integer counts, t-major, every product and sum rounded on its own; the budget is max_cost_share * (H *
//     cost[T-1][0]), two rounded products in that order -- contraction is off for the whole file.
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
constexpr int MAX_PAIRS = MAX_TIERS * 3;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int R_PASSES = 32;   // the pattern of r: 31 halvings of 0 .. 0x7f800000, and one to spare
constexpr int M_PASSES = 11;   // the head index of the partial step: 0 .. 1024
constexpr uint32_t INF_BITS = 0x7f800000u;

struct BParams {
  const float* sq_ref; const float* sq_err;
  int H, n_tiers, exact_tier;
  double budget;
  double cost[MAX_PAIRS];   // [t * 3 + e] = work[e] * tier_cost[t], formed on the host side of the launch: one rounded product
  int order[MAX_PAIRS];     // the pairs of the call by (cost, tier, -expert) ascending: the first within a bound is the head's
  int klass[MAX_PAIRS];     // [pair] = its rank among the DISTINCT costs: strictly cheaper <=> a smaller klass
  int32_t* expert; int32_t* tier; int32_t* lists; int32_t* counts; float* cost_share; float* level;
};

// the head's pair at bound r: the cheapest candidate with rel <= r (NaN meets no bound), else full attention in the last tier
__device__ __forceinline__ int pair_at(const float (*rel)[MAX_HEADS], const BParams& p, int n_pairs, int h, float r) {
  int best = (p.n_tiers - 1) * 3;
  for (int i = n_pairs - 1; i >= 0; --i) {
    const int c = p.order[i];
    if (rel[c][h] <= r) best = c;
  }
  return best;
}

// nine counts of at most 1024 in two 64-bit words, 12 bits each: pairs 0..4 and pairs 5..8
struct Counts {
  unsigned long long lo, hi;
  __device__ __forceinline__ void add(int pair) {
    if (pair < 5) lo += 1ull << (12 * pair);
    else hi += 1ull << (12 * (pair - 5));
  }
  __device__ __forceinline__ int of(int pair) const {
    return (int)(((pair < 5) ? (lo >> (12 * pair)) : (hi >> (12 * (pair - 5)))) & 0xfffull);
  }
};

// the workgroup's sum of every lane's counts, in every lane: a wave reduction, then the four waves' words through LDS.
// `slot` alternates between two buffers from pass to pass, so one barrier per pass orders the writes after the last reads
__device__ __forceinline__ Counts reduce_counts(Counts c, unsigned long long (*part)[WAVES][2], int slot) {
  for (int off = 32; off > 0; off >>= 1) {
    c.lo += __shfl_xor(c.lo, off);
    c.hi += __shfl_xor(c.hi, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[slot][wave][0] = c.lo;
    part[slot][wave][1] = c.hi;
  }
  __syncthreads();
  Counts all{0ull, 0ull};
  for (int w = 0; w < WAVES; ++w) {
    all.lo += part[slot][w][0];
    all.hi += part[slot][w][1];
  }
  return all;
}

// cost of a table from its integer counts, t-major; an empty list adds nothing, whatever its cost
__device__ __forceinline__ double cost_of(const Counts& n, const BParams& p, int n_pairs) {
  double sum = 0.0;
  for (int i = 0; i < n_pairs; ++i) {
    const int k = n.of(i);
    if (k) sum = sum + (double)k * p.cost[i];
  }
  return sum;
}

__global__ __launch_bounds__(THREADS) void route_budget_tiers_kernel(const BParams p) {
  __shared__ float s_rel[MAX_PAIRS][MAX_HEADS];            // rel of every (pair, head); -0 stored as +0
  __shared__ int s_pair[MAX_HEADS];                        // tier * 3 + expert of every head, as routed
  __shared__ unsigned long long s_part[2][WAVES][2];
  __shared__ uint32_t s_max[WAVES][2];
  const int tid = threadIdx.x;
  const int H = p.H, T = p.n_tiers, n_pairs = T * 3;
  for (int h = tid; h < H; h += THREADS) {
    const float ref = p.sq_ref[h];
    for (int t = 0; t < T; ++t) {
      const float* err = p.sq_err + ((size_t)t * H + h) * 3;
      for (int e = 0; e < 3; ++e) {
        float rel = (e == 0 && t == p.exact_tier) ? 0.f : vorta_route::rel_error(err[e == 0 ? 2 : e - 1], ref);
        if (rel == 0.f) rel = 0.f;  // (-0 is the level 0)
        s_rel[t * 3 + e][h] = rel;
      }
    }
  }
  __syncthreads();

  // 1. r*: the smallest pattern whose state is within the budget; INF_BITS where no level is
  uint32_t lo = 0u, hi = INF_BITS;
  for (int pass = 0; pass < R_PASSES; ++pass) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const float r = __uint_as_float(mid);
    Counts c{0ull, 0ull};
    for (int h = tid; h < H; h += THREADS) c.add(pair_at(s_rel, p, n_pairs, h, r));
    const Counts n = reduce_counts(c, s_part, pass & 1);
    const bool within = !(cost_of(n, p, n_pairs) > p.budget);
    if (lo < hi) {  // (the same in every lane: the counts are the workgroup's)
      if (within) hi = mid;
      else lo = mid + 1u;
    }
  }
  const bool ran_out = hi == INF_BITS;

  // 2. the largest level below r*, and the largest level (0 is always a level)
  uint32_t below = 0u, top = 0u;
  for (int h = tid; h < H; h += THREADS)
    for (int i = 0; i < n_pairs; ++i) {
      const uint32_t bits = __float_as_uint(s_rel[i][h]);
      if (bits < INF_BITS) {  // finite and not negative (a NaN's pattern, whatever its sign, is above +inf's)
        top = bits > top ? bits : top;
        if (bits < hi) below = bits > below ? bits : below;
      }
    }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t b = __shfl_xor(below, off), t = __shfl_xor(top, off);
    below = b > below ? b : below;
    top = t > top ? t : top;
  }
  if ((tid & 63) == 0) {
    s_max[tid >> 6][0] = below;
    s_max[tid >> 6][1] = top;
  }
  __syncthreads();
  below = top = 0u;
  for (int w = 0; w < WAVES; ++w) {
    below = s_max[w][0] > below ? s_max[w][0] : below;
    top = s_max[w][1] > top ? s_max[w][1] : top;
  }
  // where the candidates ran out the result is state(largest level); at r* == 0 it is state(0): no partial step in either
  const uint32_t star = ran_out ? top : hi;
  const float r_star = __uint_as_float(star);
  const float r_prev = __uint_as_float((ran_out || star == 0u) ? star : below);

  // 3. the partial step: the smallest m such that moving the heads below m leaves the cost within the budget
  int pa[MAX_HEADS / THREADS], pb[MAX_HEADS / THREADS];  // this lane's heads at r- and at r*
#pragma unroll
  for (int j = 0; j < MAX_HEADS / THREADS; ++j) {
    const int h = tid + j * THREADS;
    pa[j] = pb[j] = 0;
    if (h < H) {
      pa[j] = pair_at(s_rel, p, n_pairs, h, r_prev);
      const int b = pair_at(s_rel, p, n_pairs, h, r_star);
      pb[j] = p.klass[b] < p.klass[pa[j]] ? b : pa[j];  // (an equal cost moves no head)
    }
  }
  int m_lo = 0, m_hi = H;
  for (int pass = 0; pass < M_PASSES; ++pass) {
    const int mid = (m_lo + m_hi) >> 1;
    Counts c{0ull, 0ull};
#pragma unroll
    for (int j = 0; j < MAX_HEADS / THREADS; ++j) {
      const int h = tid + j * THREADS;
      if (h < H) c.add(h < mid ? pb[j] : pa[j]);
    }
    const Counts n = reduce_counts(c, s_part, pass & 1);
    const bool within = !(cost_of(n, p, n_pairs) > p.budget);
    if (m_hi - m_lo > 1) {
      if (within) m_hi = mid;
      else m_lo = mid;
    }
  }

  Counts c{0ull, 0ull};
#pragma unroll
  for (int j = 0; j < MAX_HEADS / THREADS; ++j) {
    const int h = tid + j * THREADS;
    if (h < H) {
      const int pair = h < m_hi ? pb[j] : pa[j];
      c.add(pair);
      s_pair[h] = pair;
      p.expert[h] = pair % 3;
      p.tier[h] = pair / 3;
    }
  }
  const Counts n = reduce_counts(c, s_part, M_PASSES & 1);  // (its barrier orders s_pair before the lists)
  if (tid < n_pairs) {  // one lane per (tier, expert) list, [n_tiers][3][heads]
    int k = 0;
    for (int h = 0; h < H; ++h)
      if (s_pair[h] == tid) p.lists[(size_t)tid * H + k++] = h;
    p.counts[tid] = k;
  }
  if (tid == 64) {  // (a wave of its own: the list lanes above are in wave 0)
    if (p.cost_share) *p.cost_share = (float)(cost_of(n, p, n_pairs) / ((double)H * p.cost[(T - 1) * 3]));
    if (p.level) *p.level = r_star;
  }
}

bool positive_finite(double x) { return x > 0.0 && x <= DBL_MAX; }  // (a NaN fails both)

}  // namespace

extern "C" int vorta_route_budget_tiers_args_size(void) { return (int)sizeof(vorta_route_budget_tiers_args); }

extern "C" int vorta_route_budget_tiers(const vorta_route_budget_tiers_args* a, void* hip_stream) {
  if (!a || a->struct_size != sizeof(vorta_route_budget_tiers_args)) return VORTA_EINVAL;
  if (a->heads < 1 || a->heads > MAX_HEADS) return VORTA_EINVAL;
  if (a->n_tiers < 1 || a->n_tiers > MAX_TIERS) return VORTA_EINVAL;
  if (a->exact_tier < -1 || a->exact_tier >= a->n_tiers) return VORTA_EINVAL;
  if (!a->sq_ref || !a->sq_err || !a->expert_of_head || !a->tier_of_head || !a->head_lists || !a->head_counts)
    return VORTA_EINVAL;
  if (!(a->max_cost_share > 0.0)) return VORTA_EINVAL;  // (a NaN fails every comparison; +inf is a budget nothing exceeds)
  for (int e = 0; e < 3; ++e)
    if (!positive_finite(a->work[e])) return VORTA_EINVAL;
  for (int t = 0; t < a->n_tiers; ++t)
    if (!positive_finite(a->tier_cost[t])) return VORTA_EINVAL;
  BParams p{};
  p.sq_ref = a->sq_ref; p.sq_err = a->sq_err;
  p.H = a->heads; p.n_tiers = a->n_tiers; p.exact_tier = a->exact_tier;
  const int n_pairs = a->n_tiers * 3;
  for (int t = 0; t < a->n_tiers; ++t)
    for (int e = 0; e < 3; ++e) p.cost[t * 3 + e] = a->work[e] * a->tier_cost[t];
  const double dense = (double)a->heads * p.cost[(a->n_tiers - 1) * 3];
  p.budget = a->max_cost_share * dense;
  // the pairs by (cost, tier, -expert): an insertion sort of at most nine
  for (int i = 0; i < n_pairs; ++i) p.order[i] = i;
  auto before = [&](int x, int y) {  // x's key < y's
    if (p.cost[x] != p.cost[y]) return p.cost[x] < p.cost[y];
    if (x / 3 != y / 3) return x / 3 < y / 3;
    return x % 3 > y % 3;
  };
  for (int i = 1; i < n_pairs; ++i)
    for (int j = i; j > 0 && before(p.order[j], p.order[j - 1]); --j) {
      const int s = p.order[j]; p.order[j] = p.order[j - 1]; p.order[j - 1] = s;
    }
  for (int i = 0, k = 0; i < n_pairs; ++i) {
    if (i > 0 && p.cost[p.order[i]] != p.cost[p.order[i - 1]]) ++k;
    p.klass[p.order[i]] = k;
  }
  p.expert = a->expert_of_head; p.tier = a->tier_of_head; p.lists = a->head_lists; p.counts = a->head_counts;
  p.cost_share = a->cost_share; p.level = a->level;
  hipLaunchKernelGGL(route_budget_tiers_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)hip_stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VORTA_OK : vorta_set_hip_error(e);
}
