// Host-side check of vorta_route_budget_tiers' argument validation under AddressSanitizer / UBSan, on the CPU: every refusal
// path with null and out-of-range arguments.  Nothing is launched -- every call below must return VORTA_EINVAL before the
// launcher touches a pointer -- so the program needs no GPU.  Build and run (from the repository root):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ivorta_amd/csrc \
//       vorta_amd/csrc/route_budget_tiers.hip vorta_amd/csrc/api.hip tools/sanitize_route_budget_tiers.cpp -o /tmp/san_rbt
//   /tmp/san_rbt
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vorta_hip.h"

static int failures = 0;

static void expect_einval(const vorta_route_budget_tiers_args* a, const char* what) {
  const int rc = vorta_route_budget_tiers(a, nullptr);
  if (rc != VORTA_EINVAL) {
    std::printf("FAIL %s: returned %d\n", what, rc);
    ++failures;
  }
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // host addresses that are never dereferenced on the host: a refused call reads the block alone
  static float ref[8], err[2 * 8 * 3];
  static int32_t expert[8], tier[8], lists[2 * 3 * 8], counts[2 * 3];
  vorta_route_budget_tiers_args good;
  std::memset(&good, 0, sizeof good);
  good.struct_size = (uint32_t)sizeof good;
  good.heads = 8; good.n_tiers = 2; good.exact_tier = 1;
  good.sq_ref = ref; good.sq_err = err;
  good.max_cost_share = 0.5;
  good.work[0] = 3.0; good.work[1] = 2.0; good.work[2] = 1.0;
  good.tier_cost[0] = 0.59; good.tier_cost[1] = 1.0; good.tier_cost[2] = nan;  // (the third is past n_tiers: not looked at)
  good.expert_of_head = expert; good.tier_of_head = tier; good.head_lists = lists; good.head_counts = counts;

  if (vorta_route_budget_tiers_args_size() != (int)sizeof good) {
    std::printf("FAIL args_size\n");
    ++failures;
  }
  expect_einval(nullptr, "null block");
  vorta_route_budget_tiers_args a;
#define CASE(stmt, what) a = good; stmt; expect_einval(&a, what)
  CASE(a.struct_size -= 8, "struct_size short");
  CASE(a.struct_size = 0, "struct_size 0");
  CASE(a.heads = 0, "heads 0");
  CASE(a.heads = -1, "heads -1");
  CASE(a.heads = 1025, "heads 1025");
  CASE(a.heads = std::numeric_limits<int32_t>::max(), "heads INT_MAX");
  CASE(a.heads = std::numeric_limits<int32_t>::min(), "heads INT_MIN");
  CASE(a.n_tiers = 0, "n_tiers 0");
  CASE(a.n_tiers = 4, "n_tiers 4");
  CASE(a.n_tiers = std::numeric_limits<int32_t>::max(), "n_tiers INT_MAX");
  CASE(a.n_tiers = std::numeric_limits<int32_t>::min(), "n_tiers INT_MIN");
  CASE(a.exact_tier = -2, "exact_tier -2");
  CASE(a.exact_tier = 2, "exact_tier == n_tiers");
  CASE(a.exact_tier = std::numeric_limits<int32_t>::max(), "exact_tier INT_MAX");
  CASE(a.sq_ref = nullptr, "null sq_ref");
  CASE(a.sq_err = nullptr, "null sq_err");
  CASE(a.expert_of_head = nullptr, "null expert_of_head");
  CASE(a.tier_of_head = nullptr, "null tier_of_head");
  CASE(a.head_lists = nullptr, "null head_lists");
  CASE(a.head_counts = nullptr, "null head_counts");
  CASE(a.max_cost_share = 0.0, "share 0");
  CASE(a.max_cost_share = -0.0, "share -0");
  CASE(a.max_cost_share = -0.5, "share negative");
  CASE(a.max_cost_share = -inf, "share -inf");
  CASE(a.max_cost_share = nan, "share NaN");
  for (int e = 0; e < 3; ++e) {
    CASE(a.work[e] = 0.0, "work 0");
    CASE(a.work[e] = -1.0, "work negative");
    CASE(a.work[e] = inf, "work inf");
    CASE(a.work[e] = nan, "work NaN");
  }
  for (int t = 0; t < 2; ++t) {
    CASE(a.tier_cost[t] = 0.0, "tier_cost 0");
    CASE(a.tier_cost[t] = -1.0, "tier_cost negative");
    CASE(a.tier_cost[t] = inf, "tier_cost inf");
    CASE(a.tier_cost[t] = nan, "tier_cost NaN");
  }
  CASE(a.n_tiers = 3, "third tier_cost NaN");
  CASE((a.heads = 0, a.sq_ref = nullptr, a.n_tiers = 7, a.max_cost_share = nan), "everything wrong at once");
#undef CASE
  if (failures) {
    std::printf("%d refusal(s) missing\n", failures);
    return 1;
  }
  std::printf("every refusal path returned VORTA_EINVAL\n");
  return 0;
}
