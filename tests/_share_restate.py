"""A numpy restatement of vorta_sta_select_tiles_share (include/vorta_hip.h): per head slot and query tile the fewest key
tiles, in the rank order of vorta_sta_select_tiles, whose float32 scores -- summed in float32 in rank order -- reach
float32(mass_share) * rows_per_tile, at least 1 and at most n_sel.  Nothing here reads the library."""
import numpy as np


def rank_order(row, i):
    """the tiles of one score row in rank order: tile i first, then j != i by descending score (-0 = +0, a NaN by its bits),
    equal scores to the lower j"""
    b = (np.asarray(row, np.float32) + np.float32(0)).view(np.uint32).astype(np.int64)
    key = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    rest = [j for j in np.lexsort((np.arange(len(row)), -key)) if j != i]
    return [i] + rest


def select_fixed(score, n_sel, tok, t_eff, q_rows):
    """(sel_tiles (Y,N,n_sel) ascending, kv_rows (Y,N,n_sel tok + t_eff)) of vorta_sta_select_tiles(phases = 3) without a
    row_map: the first n_sel tiles of `rank_order`, their rows through q_rows, then the text rows"""
    score = np.asarray(score, np.float32)
    Y, N = score.shape[:2]
    rows = np.asarray(q_rows).reshape(N, tok)
    text = np.arange(N * tok, N * tok + t_eff, dtype=np.int32)
    tiles = np.array([[sorted(rank_order(score[y, i], i)[:n_sel]) for i in range(N)] for y in range(Y)], np.int32)
    kv = np.concatenate([rows[tiles].reshape(Y, N, n_sel * tok), np.broadcast_to(text, (Y, N, t_eff))], -1).astype(np.int32)
    return tiles, kv


def planted_scores(slots, n_tiles, seed=11):
    """a float32 score matrix (slots, n_tiles, n_tiles) for selections over MORE than 64 key tiles (n_tiles >= 75), every entry
    a multiple of 2^-5 so that every float32 prefix sum is exact.  40 levels over 75+ tiles: every row holds equal scores.
    Rows i = 2 mod 5 hold 23 distinct positive scores, -0 at tiles 3, 66 and 74, +0 at tiles 40 and 70 and negative scores
    elsewhere: +0 and -0 must tie (to the lower tile) for the places left behind the positive ones.  One NaN off the diagonal,
    at (slot 0, row 1, tile 69): by its bits it ranks in front of every number."""
    assert n_tiles >= 75
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 40, (slots, n_tiles, n_tiles)).astype(np.float32) / 32
    zeros = {3: -0.0, 40: 0.0, 66: -0.0, 70: 0.0, 74: -0.0}
    free = np.array([j for j in range(n_tiles) if j not in zeros])
    for y in range(slots):
        for i in range(2, n_tiles, 5):
            s[y, i] = -(1 + s[y, i])
            s[y, i, rng.choice(free, 23, replace=False)] = (1 + rng.permutation(23)).astype(np.float32) / 32
            for j, z in zeros.items():
                s[y, i, j] = z
    s[0, 1, 69] = np.nan
    return s


def straddles(tiles, at=64):
    """per slot: whether some row of the kept tiles (Y,N,n_sel; -1 = unused) holds tiles below AND at or above `at` -- what
    makes the second 64-lane pass of the selection, and the count it carries over, show in the result"""
    t = np.asarray(tiles)
    return ((((t >= 0) & (t < at)).any(-1)) & ((t >= at).any(-1))).any(-1)


def select_share(score, mass_share, rows_per_tile, n_sel, tok, t_eff, q_rows, strict=False):
    """(sel_count (Y,N), sel_tiles (Y,N,n_sel) ascending then -1, kv_len (Y,N), lists: [y][i] = the key rows of the list).
    strict: assert that no prefix sum EQUALS the threshold (a case then rests on no rounding)"""
    score = np.asarray(score, np.float32)
    Y, N = score.shape[:2]
    thr = np.float32(mass_share) * np.float32(rows_per_tile)
    rows = np.asarray(q_rows).reshape(N, tok)
    text = np.arange(N * tok, N * tok + t_eff, dtype=np.int32)
    count, tiles, lists = np.zeros((Y, N), np.int32), np.full((Y, N, n_sel), -1, np.int32), []
    for y in range(Y):
        lists.append([])
        for i in range(N):
            order, s, c = rank_order(score[y, i], i), np.float32(0), n_sel
            for r in range(n_sel):
                s = np.float32(s + score[y, i, order[r]])
                assert not (strict and s == thr), "a prefix sum equals the threshold"
                if s >= thr:
                    c = r + 1
                    break
            count[y, i] = c
            tiles[y, i, :c] = sorted(order[:c])
            lists[y].append(np.concatenate([rows[tiles[y, i, :c]].reshape(-1), text]).astype(np.int32))
    return count, tiles, count * tok + t_eff, lists
