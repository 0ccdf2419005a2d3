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
