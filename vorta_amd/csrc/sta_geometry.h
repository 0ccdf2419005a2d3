// The dividing sliding-tile geometry the key-tile selection (sta_select.hip) and its mass statistic (sta_mass.hip) share.
#pragma once
#include <stdint.h>

#include "vorta_hip.h"

namespace vorta_sta {

constexpr int MAX_TILES = 1024;  // keys and lists of a selecting wave live in LDS

struct Geometry { int S, tok, n_tiles, n_sel; };

// n_tiles, tok and n_sel = cnt_0 cnt_1 cnt_2 as vorta_sta_build_tables; VORTA_EINVAL for a tile that does not divide
inline int geometry(const int32_t* latent, const int32_t* tile, const int32_t* window, int32_t t_eff, Geometry& g) {
  int64_t S = 1, tok = 1, n_tiles = 1, n_sel = 1;
  for (int d = 0; d < 3; ++d) {
    if (latent[d] <= 0 || tile[d] <= 0 || window[d] <= 0) return VORTA_EINVAL;
    if (latent[d] % tile[d]) return VORTA_EINVAL;  // a dividing geometry, as vorta_sta_build_tables
    const int nt = latent[d] / tile[d];
    const int cnt = 2 * (window[d] / 2) + 1;
    S *= latent[d]; tok *= tile[d]; n_tiles *= nt;
    n_sel *= nt < cnt ? nt : cnt;
  }
  if (t_eff < 0 || S + t_eff > 0x7fffffff || n_sel * tok + t_eff > 0x7fffffff) return VORTA_EINVAL;
  g.S = (int)S; g.tok = (int)tok; g.n_tiles = (int)n_tiles; g.n_sel = (int)n_sel;
  return VORTA_OK;
}

}  // namespace vorta_sta
