"""GPU: vorta_sta_select_tiles (csrc/sta_select.hip) -- the sliding-tile expert's key tiles chosen by content -- against the
rule in float64 on the same 16-bit inputs: tile i itself and the n_sel - 1 tiles j != i of highest <mean q_i, mean k_j>, ties
to the lower j, ascending; kv_rows = their rows through q_rows, then the text rows.

The kernel sums in fp32, so a selection may differ from float64 where two scores are closer than the rounding of either:
eps_i = (2 tok + 128 + 4) 2^-24 max_j sum_d mean|q|[i][d] mean|k|[j][d] (an fp32 sum of tok terms, then a 128-term dot).  Every
case first asserts, from the reference alone, that the last selected and the first unselected score of every row are more than
2 eps apart (the seeds are chosen so); then the lists must be EQUAL.

One geometry: latent (10,6,8), tile (2,3,4): 20 tiles (not a multiple of 32 or of the 4 query tiles of a workgroup) of 24 rows
(not a multiple of the 16 rows of a pass).  Then the selection tail alone over MORE than 64 key tiles (80 and 75), on score
matrices written into ws, against the integer restatement of tests/_share_restate.py."""
import numpy as np
import pytest
import torch

from _util import dev

pytestmark = pytest.mark.gpu

LATENT, TILE, TOK, N_TILES, S, H = (10, 6, 8), (2, 3, 4), 24, 20, 480, 3
N_ROWS = S + 5 + 11  # rows of q and k: video, text and rows only a row_map reaches
WINDOWS = {1: (1, 1, 1), 6: (3, 3, 1), 20: (5, 3, 3)}  # n_sel -> window: the own tile only, an interior count, every tile
FILL = -7
# (seeds: the first for which the precondition of _reference holds in the case that uses them; checked on the CPU)


def _reference(q, k, q_rows, n_sel, heads):
    """(sel_tiles (slots, 20, n_sel) of the rule in float64; asserts the near-tie precondition)"""
    qt, kt = (x.double().cpu()[heads][:, q_rows.cpu().long()].view(len(heads), N_TILES, TOK, 128) for x in (q, k))
    score = qt.mean(2) @ kt.mean(2).transpose(1, 2)
    eps = (2 * TOK + 128 + 4) * 2.0 ** -24 * (qt.abs().mean(2) @ kt.abs().mean(2).transpose(1, 2)).amax(-1)
    own = torch.arange(N_TILES)
    score[:, own, own] = float("inf")  # the tile itself is always selected
    order = torch.argsort(score, dim=-1, descending=True, stable=True)  # (stable: equal scores go to the lower j)
    if 1 < n_sel < N_TILES:
        ranked = score.gather(-1, order)
        gap = ranked[..., n_sel - 1] - ranked[..., n_sel]
        assert (gap > 2 * eps).all(), f"near tie: gap / eps min {float((gap / eps).min()):.2f} (choose another seed)"
    return order[..., :n_sel].sort(-1).values.to(torch.int32)


def _inputs(dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((H, N_ROWS, 128), generator=gen).to(dtype).to(dev()) for _ in range(2))


def _run(q, k, n_sel, t_eff, row_map=None, head_list=None, n_heads_dev=None):
    from vorta_amd import ops
    window = WINDOWS[n_sel]
    q_rows, _ = ops.sta_build_tables(LATENT, TILE, window, t_eff, dev(), row_map=row_map)
    n_slots = H if head_list is None else head_list.numel()
    bufs = ops.sta_select_buffers(n_slots, N_TILES, n_sel, n_sel * TOK + t_eff, dev())
    for b in bufs[:2]:
        b.fill_(FILL)
    kv, sel, n_kv = ops.sta_select_tiles(q, k, LATENT, TILE, window, t_eff, q_rows, head_list=head_list,
                                         n_heads_dev=n_heads_dev, row_map=row_map, out=bufs)
    torch.cuda.synchronize()
    assert n_kv == n_sel * TOK + t_eff and tuple(kv.shape) == (n_slots, N_TILES, n_kv)
    live = n_slots if n_heads_dev is None else int(n_heads_dev.item())
    heads = list(range(H)) if head_list is None else head_list.tolist()
    want = _reference(q, k, q_rows, n_sel, heads[:live])
    assert torch.equal(sel[:live].cpu(), want), "sel_tiles differs from the float64 rule"
    # kv_rows: the expansion of sel_tiles through q_rows, then the text rows
    video = q_rows.cpu().view(N_TILES, TOK)[want.long()].reshape(live, N_TILES, n_sel * TOK)
    text = torch.arange(S, S + t_eff, dtype=torch.int32)
    if row_map is not None:
        text = row_map.cpu()[text.long()]
    assert torch.equal(kv[:live].cpu(), torch.cat([video, text.expand(live, N_TILES, t_eff)], dim=-1))
    assert (kv[live:] == FILL).all() and (sel[live:] == FILL).all(), "slots past the device count were written"
    return want


@pytest.mark.parametrize("t_eff", [0, 5])
@pytest.mark.parametrize("n_sel", list(WINDOWS))
@pytest.mark.parametrize("dtype,seed", [(torch.bfloat16, 7), (torch.float16, 7)], ids=["bf16", "fp16"])
def test_selection_matches_float64(dtype, seed, n_sel, t_eff):
    q, k = _inputs(dtype, seed)
    _run(q, k, n_sel, t_eff)


def test_head_list_with_a_device_count_leaves_trailing_slots_alone():
    q, k = _inputs(torch.bfloat16, 6)
    _run(q, k, 6, 5, head_list=torch.tensor([2, 0, 1], dtype=torch.int32, device=dev()),
         n_heads_dev=torch.tensor([2], dtype=torch.int32, device=dev()))


def test_row_map():
    """token i lives in physical row row_map[i] of q and k (a permutation into a longer buffer): the means follow q_rows, the
    lists hold physical rows, the text rows included"""
    row_map = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(4))[:S + 5].to(torch.int32).to(dev())
    q, k = _inputs(torch.float16, 1)
    _run(q, k, 6, 5, row_map=row_map)


WIDE = {80: (10, 8, 8), 75: (10, 6, 10)}  # n_tiles -> latent at tile (2,2,2): a multiple of a workgroup's 4 tiles; one idle wave
WIDE_TILE, WIDE_WINDOW, WIDE_TOK, WIDE_N_SEL, WIDE_SLOTS = (2, 2, 2), (3, 3, 3), 8, 27, 2


def wide_tables(n_tiles, t_eff, score):
    """(q_rows, the `sta_share_buffers` of the WIDE geometry with `score` written where the statistic leaves its matrix)"""
    from vorta_amd import ops
    q_rows, _ = ops.sta_build_tables(WIDE[n_tiles], WIDE_TILE, WIDE_WINDOW, t_eff, dev())
    tabs = ops.sta_share_buffers(WIDE_SLOTS, n_tiles, WIDE_N_SEL, WIDE_N_SEL * WIDE_TOK + t_eff, dev(), WIDE_TOK, 1)
    for x in tabs[:5]:
        x.fill_(FILL)
    tabs.ws[:score.size] = torch.as_tensor(score.reshape(-1), device=dev())
    return q_rows, tabs


def wide_select(n_tiles, t_eff, q_rows, tabs):
    """`sta_select_tiles(phases=3)` over the matrix in tabs.ws, into tables of its own: (kv_rows, sel_tiles)"""
    from vorta_amd import ops
    n_kv = WIDE_N_SEL * WIDE_TOK + t_eff
    kv, sel, ws = ops.sta_select_buffers(WIDE_SLOTS, n_tiles, WIDE_N_SEL, n_kv, dev(), "mass", WIDE_TOK)
    for b in (kv, sel):
        b.fill_(FILL)
    ws[:WIDE_SLOTS * n_tiles * n_tiles] = tabs.ws[:WIDE_SLOTS * n_tiles * n_tiles]
    dummy = torch.zeros((WIDE_SLOTS, 1, 128), dtype=torch.bfloat16, device=dev())  # (phases 3 reads neither q nor k)
    ops.sta_select_tiles(dummy, dummy, WIDE[n_tiles], WIDE_TILE, WIDE_WINDOW, t_eff, q_rows, out=(kv, sel, ws), phases=3)
    torch.cuda.synchronize()
    return kv, sel


@pytest.mark.parametrize("t_eff", [0, 5])
@pytest.mark.parametrize("n_tiles", list(WIDE))
def test_more_than_64_key_tiles(n_tiles, t_eff):
    """both 64-lane passes of the rank and of the ascending list, and the count the list carries from one pass to the next:
    80 and 75 key tiles of 8 rows, n_sel = 27, a score matrix written into ws (ties in every row, +0 / -0, a NaN), the fixed
    count and the share selection (mass_share 0.5 of 8 sampled rows) against tests/_share_restate.py as integers"""
    import _share_restate as R
    from vorta_amd import ops
    score = R.planted_scores(WIDE_SLOTS, n_tiles)
    q_rows, tabs = wide_tables(n_tiles, t_eff, score)
    rows = q_rows.cpu().numpy()
    tiles, lists = R.select_fixed(score, WIDE_N_SEL, WIDE_TOK, t_eff, rows)
    count, s_tiles, kv_len, s_lists = R.select_share(score, 0.5, WIDE_TOK, WIDE_N_SEL, WIDE_TOK, t_eff, rows)
    # a condition on the inputs: in every slot some row keeps tiles on both sides of tile 64, under either selection
    assert R.straddles(tiles).all() and R.straddles(s_tiles).all()
    assert count.min() < WIDE_N_SEL and count.max() == WIDE_N_SEL  # (short lists, and the NaN row's full one)

    kv, sel = wide_select(n_tiles, t_eff, q_rows, tabs)
    assert (sel.cpu().numpy() == tiles).all(), "sel_tiles differs from the rank order"
    assert (kv.cpu().numpy() == lists).all(), "kv_rows is not the kept tiles' rows through q_rows, then the text rows"

    ops.sta_select_tiles_share(WIDE[n_tiles], WIDE_TILE, WIDE_WINDOW, t_eff, q_rows, tabs, mass_share=0.5, n_heads=WIDE_SLOTS,
                               rows_per_tile=WIDE_TOK, block_rows=128)
    torch.cuda.synchronize()
    kv, sel, cnt, length, order, _ = (x.cpu().numpy() for x in tabs)
    assert (cnt == count).all() and (sel == s_tiles).all() and (length == kv_len).all()
    for y in range(WIDE_SLOTS):
        for i in range(n_tiles):
            assert (kv[y, i, :kv_len[y, i]] == s_lists[y][i]).all(), (y, i)
            assert (kv[y, i, (kv_len[y, i] + 3) // 4 * 4:] == FILL).all(), "written behind the list's length rounded up to 4"
    assert sorted(order.tolist()) == list(range(WIDE_SLOTS * n_tiles))
    assert (np.diff(count.reshape(-1)[order]) <= 0).all(), "order: tile counts must not increase"


def test_planted_far_tile_is_selected():
    """k of tile j lies along axis j (scaled, distinct), q of tile i along axis (i + 9) % 20, over small noise: whatever the
    window would hold, row i's list holds that far tile"""
    from vorta_amd import ops
    q, k = (0.05 * x.float().cpu() for x in _inputs(torch.bfloat16, 2))
    q_rows, _ = ops.sta_build_tables(LATENT, TILE, WINDOWS[6], 0, dev())
    tile_of_row = torch.empty(S, dtype=torch.long)
    tile_of_row[q_rows.cpu().long()] = torch.arange(S) // TOK
    far = (torch.arange(N_TILES) + 9) % N_TILES
    k[:, torch.arange(S), tile_of_row] += 2.0 + 0.1 * tile_of_row
    q[:, torch.arange(S), far[tile_of_row]] += 1.0
    want = _run(q.to(torch.bfloat16).to(dev()), k.to(torch.bfloat16).to(dev()), 6, 0)
    assert (want == far.to(torch.int32)[None, :, None]).any(-1).all()
