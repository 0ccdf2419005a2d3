"""Partial geometry, restated from its definition (DESIGN.md "Partial geometry") in numpy float64 -- never from the table code.

Everything is computed per token from its (frame, row, column) coordinates: which tile and which coreset window a token is
in, and for every (query token, key token) pair whether the sliding-tile expert lets the query see the key.  The experts are
then MASKED DENSE attention over all S + T rows: a boolean (N, N) mask per head, softmax over the visible keys, and -- for
the coreset expert -- a source map that copies a centre's output row into the dropped margins of its window.

`expert_specs` gives (mask, src) per expert; `attend` evaluates one in numpy, `attend_torch` is the same arithmetic in torch
(any dtype, differentiable) for the backward tests."""
import math

import numpy as np


def coords(latent):
    """(S, 3) int: the (frame, row, column) of every token, raster order"""
    return np.stack(np.meshgrid(*[np.arange(n) for n in latent], indexing="ij"), -1).reshape(-1, 3)


def n_tiles(latent, tile):
    return tuple(-(-l // t) for l, t in zip(latent, tile))


def tile_id(latent, tile):
    """(S,) the raster id, on the tile grid, of the tile [i*tile, min((i+1)*tile, latent)) a token lies in"""
    nt = n_tiles(latent, tile)
    t3 = coords(latent) // np.asarray(tile)
    return (t3[:, 0] * nt[1] + t3[:, 1]) * nt[2] + t3[:, 2]


def tile_major_order(latent, tile):
    """token at tile-major position i: tiles in raster order of the tile grid; inside a tile raster order of its own box,
    which for an axis-aligned box is ascending token id"""
    tid = tile_id(latent, tile)
    return np.lexsort((np.arange(tid.size), tid))


def window_first_count(latent, tile, window):
    """per dimension: (first[t] for every tile t, cnt) -- centre = min(max(t, half), nt-1-half), first = max(centre-half, 0),
    cnt = min(nt, 2 half + 1)"""
    out = []
    for d, nt in enumerate(n_tiles(latent, tile)):
        half = window[d] // 2
        first = [max(min(max(t, half), nt - 1 - half) - half, 0) for t in range(nt)]
        out.append((np.asarray(first), min(nt, 2 * half + 1)))
    return out


def sta_visible(latent, tile, window):
    """(S, S) bool: may query token i see key token j under the sliding-tile expert?"""
    t3 = coords(latent) // np.asarray(tile)
    ok = np.ones((t3.shape[0], t3.shape[0]), dtype=bool)
    for d, (first, cnt) in enumerate(window_first_count(latent, tile, window)):
        f = first[t3[:, d]][:, None]
        ok &= (t3[None, :, d] >= f) & (t3[None, :, d] < f + cnt)
    return ok


def sta_tile_visible(latent, tile, window):
    """(n_tiles, n_tiles) bool on the tile grid (comparable with the oracle's sta_window_tiles on dividing geometries)"""
    tid = tile_id(latent, tile)
    vis = sta_visible(latent, tile, window)
    rep = np.asarray([np.nonzero(tid == t)[0][0] for t in range(tid.max() + 1)])
    return vis[rep][:, rep]


def key_list_lengths(latent, tile, window):
    """the distinct numbers of video keys a query token sees, derived per dimension: a window that reaches the thin last tile
    is shorter than one that does not"""
    per_dim = []
    for d, (first, cnt) in enumerate(window_first_count(latent, tile, window)):
        per_dim.append({min((f + cnt) * tile[d], latent[d]) - f * tile[d] for f in first})
    return sorted({a * b * c for a in per_dim[0] for b in per_dim[1] for c in per_dim[2]})


class Coreset:
    """windows of the cropped box (ng = floor(latent / group) per dimension), from coordinates:
    centres (G,), margins (G, g-1) in in-window raster order, remainder (C,) ascending, role (S,) in {0 centre, 1 margin,
    2 remainder}, window (S,) the window id of a token (-1 for the remainder)"""

    def __init__(self, latent, group, rate=0.5):
        c = coords(latent)
        grp = np.asarray(group)
        ng = np.asarray(latent) // grp
        if (ng == 0).any():
            raise ValueError("no whole window")
        inside = (c < ng * grp).all(1)
        w3, l3 = c // grp, c % grp
        wid = (w3[:, 0] * ng[1] + w3[:, 1]) * ng[2] + w3[:, 2]
        lid = (l3[:, 0] * grp[1] + l3[:, 1]) * grp[2] + l3[:, 2]
        is_centre = inside & (l3 == grp // 2).all(1)
        self.g = int(grp.prod())
        self.G = int(ng.prod())
        self.n_keep = int(self.g * (1 - rate)) - 1
        self.S = c.shape[0]
        self.remainder = np.nonzero(~inside)[0]
        self.C = self.remainder.size
        self.S_low = self.G * (1 + self.n_keep) + self.C
        self.role = np.where(~inside, 2, np.where(is_centre, 0, 1))
        self.window = np.where(inside, wid, -1)
        self.centres = np.full(self.G, -1)
        self.margins = [[] for _ in range(self.G)]
        for tok in np.lexsort((lid, wid)):  # window by window, in-window raster order
            if not inside[tok]:
                continue
            if is_centre[tok]:
                self.centres[wid[tok]] = tok
            else:
                self.margins[wid[tok]].append(tok)
        self.margins = np.asarray(self.margins).reshape(self.G, self.g - 1)

    def keep_layout(self, kept, T=0):
        """the keep list [G centres | G*n_keep kept margins | C remainder ascending | T text] for kept (G, n_keep) token ids"""
        return np.concatenate([self.centres, np.asarray(kept).reshape(-1), self.remainder, self.S + np.arange(T)])

    def unpool_src(self, kept, N):
        """(N,) source row of every output row: a dropped margin reads its window's centre, every other row itself"""
        src = np.arange(N)
        kept = np.asarray(kept)
        for w in range(self.G):
            for tok in self.margins[w]:
                if tok not in kept[w]:
                    src[tok] = self.centres[w]
        return src


def expert_specs(latent, tile, window, cs, kept_q, kept_k, T=0, te=0):
    """per expert (full, coreset, sliding): (mask (H, N, N) bool, src (H, N) int).  kept_q / kept_k: (H, G, n_keep) token ids of
    the kept margins on the query and on the key side (the ranking is not restated: the kernel's own choice is handed in).
    Row i of a mask all False = an output row of zeros (padded text)."""
    S = cs.S
    N = S + T
    H = len(kept_q)
    valid = np.arange(N) < S + te
    full = np.broadcast_to(valid[:, None] & valid[None, :], (H, N, N)).copy()
    sl = np.zeros((N, N), dtype=bool)
    sl[:S, :S] = sta_visible(latent, tile, window)
    sl[:S, S:S + te] = True
    sl[S:S + te, :S + te] = True
    ident = np.broadcast_to(np.arange(N), (H, N)).copy()
    low, src = np.zeros((H, N, N), dtype=bool), np.zeros((H, N), dtype=np.int64)
    for h in range(H):
        keys = np.zeros(N, dtype=bool)
        keys[cs.centres] = keys[cs.remainder] = True
        keys[np.asarray(kept_k[h]).reshape(-1)] = True
        keys[S:S + te] = True
        low[h] = valid[:, None] & keys[None, :]  # (rows of dropped margins are computed and then overwritten by `src`)
        src[h] = cs.unpool_src(kept_q[h], N)
    return [(full, ident), (low, src), (np.broadcast_to(sl, (H, N, N)).copy(), ident)]


def attend(q, k, v, mask, src, scale=None):
    """(H, N, D) float64: softmax over the visible keys, zero rows where nothing is visible, then out[h] = out[h][src[h]]"""
    q, k, v = (np.asarray(x, dtype=np.float64) for x in (q, k, v))
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = np.where(mask, np.matmul(q, np.swapaxes(k, -1, -2)) * scale, -np.inf)
    mx = s.max(-1, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(mx), mx, 0.0))
    den = p.sum(-1, keepdims=True)
    o = np.matmul(np.divide(p, den, out=np.zeros_like(p), where=den > 0), v)
    return np.take_along_axis(o, src[:, :, None], axis=1)


def mixture(q, k, v, scores, specs):
    """sum_e scores[h, e] * expert_e"""
    sc = np.asarray(scores, dtype=np.float64)
    return sum(sc[:, e, None, None] * attend(q, k, v, *specs[e]) for e in range(3))


def attend_torch(q, k, v, mask, src, scale=None):
    """`attend` in torch, in the dtype of q (matmul and softmax in that dtype), differentiable"""
    import torch
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    m = torch.as_tensor(mask, device=q.device)
    s = ((q @ k.transpose(1, 2)) * scale).masked_fill(~m, float("-inf"))
    live = m.any(-1, keepdim=True)
    p = torch.softmax(torch.where(live, s, torch.zeros_like(s)), dim=-1)
    o = torch.where(live, p @ v, torch.zeros_like(q))
    idx = torch.as_tensor(src, device=q.device)[:, :, None].expand(-1, -1, q.shape[-1])
    return torch.gather(o, 1, idx)


def mixture_torch(q, k, v, scores, specs):
    return sum(scores[:, e, None, None] * attend_torch(q, k, v, *specs[e]) for e in range(3))
