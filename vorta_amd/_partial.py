"""The process-wide switch for tile and coreset windows that do not divide the latent grid (DESIGN.md "Partial geometry").
Off (the default): every routed path refuses such a geometry with the reference's messages.  On: the refusing call sites
accept it and `RoutedGeometry` builds the partial tables.  A geometry that divides is built the same way either way."""
import os
from typing import Optional

_partial_geometry: Optional[bool] = None  # None = not set: VORTA_PARTIAL_GEOMETRY, else off


def set_partial_geometry(on: bool) -> None:
    """overrides the environment switch VORTA_PARTIAL_GEOMETRY=0|1; read when a geometry is validated or built"""
    global _partial_geometry
    _partial_geometry = bool(on)


def partial_geometry() -> bool:
    if _partial_geometry is not None:
        return _partial_geometry
    env = os.environ.get("VORTA_PARTIAL_GEOMETRY", "0")
    if env not in ("", "0", "1"):
        raise ValueError(f"VORTA_PARTIAL_GEOMETRY={env!r}: 0 or 1")
    return env == "1"


def divides(latent, tile=(1, 1, 1), group=None) -> bool:
    """whether the tile and (if given) the coreset window divide the latent grid: the geometry of every earlier build"""
    return all(int(l) % int(t) == 0 for l, t in zip(latent, tile)) and \
        (group is None or all(int(l) % int(w) == 0 for l, w in zip(latent, group)))


def check_windows(latent, group) -> None:
    """a partial geometry still needs one whole coreset window per dimension (G > 0)"""
    if any(int(l) < int(w) for l, w in zip(latent, group)):
        raise ValueError(f"Low-res window {tuple(group)} holds no whole window in latent shape {tuple(latent)}.")


def window_geometry(latent, tile, window):
    """The sliding-tile window rule on the tile grid, per dimension: tiles nt = ceil(latent / tile), window tiles
    cnt = min(nt, 2 half + 1), and for every tile t the first tile of its clamped window (csrc/sta_tables.hip:
    centre = min(max(t, half), nt - 1 - half), first = max(centre - half, 0)).  Host integers; the one host copy of the rule."""
    nt = [-(-int(l) // int(t)) for l, t in zip(latent, tile)]
    cnt = [min(n, 2 * (int(w) // 2) + 1) for n, w in zip(nt, window)]
    first = []
    for d in range(3):
        half = int(window[d]) // 2
        first.append([max(min(max(t, half), nt[d] - 1 - half) - half, 0) for t in range(nt[d])])
    return nt, cnt, first


def list_extent(latent, tile, d: int, f: int, cnt: int) -> int:
    """tokens along dimension d of the window whose first tile is f: its tiles are neighbours, the last may be thin"""
    return min((f + cnt) * int(tile[d]), int(latent[d])) - f * int(tile[d])


def sliding_key_counts(latent, tile, window) -> list:
    """the distinct VIDEO key counts of the sliding expert's key lists, longest first (at most two extents per dimension)"""
    nt, cnt, first = window_geometry(latent, tile, window)
    per_dim = [sorted({list_extent(latent, tile, d, f, cnt[d]) for f in first[d]}) for d in range(3)]
    return sorted({a * b * c for a in per_dim[0] for b in per_dim[1] for c in per_dim[2]}, reverse=True)


def sliding_video_pairs(latent, tile, window) -> int:
    """(video query, video key) pairs of the sliding expert: the sum over query tokens of the video keys each sees.  The rule
    is separable, so it is a product over the dimensions of sum_t thickness(t) * extent(first(t)); S * n_kv where the tile
    divides the grid."""
    nt, cnt, first = window_geometry(latent, tile, window)
    pairs = 1
    for d in range(3):
        pairs *= sum(min(int(tile[d]), int(latent[d]) - t * int(tile[d])) * list_extent(latent, tile, d, first[d][t], cnt[d])
                     for t in range(nt[d]))
    return pairs


def coreset_numbers(latent, group, rate):
    """(G, n_keep, C, S_low): whole windows of the cropped box, kept margins per window (coreset_select.py:54), tokens outside
    the box (full resolution), rows of the coreset sequence G (1 + n_keep) + C.  C = 0 where the window divides the grid."""
    check_windows(latent, group)
    g = int(group[0]) * int(group[1]) * int(group[2])
    G = 1
    for l, w in zip(latent, group):
        G *= int(l) // int(w)
    n_keep = int(g * (1 - float(rate))) - 1
    C = int(latent[0]) * int(latent[1]) * int(latent[2]) - G * g
    return G, n_keep, C, G * (1 + n_keep) + C
