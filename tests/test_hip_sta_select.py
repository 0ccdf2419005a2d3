"""GPU: vorta_sta_select_tiles (csrc/sta_select.hip) -- the sliding-tile expert's key tiles chosen by content -- against the
rule in float64 on the same 16-bit inputs: tile i itself and the n_sel - 1 tiles j != i of highest <mean q_i, mean k_j>, ties
to the lower j, ascending; kv_rows = their rows through q_rows, then the text rows.

The kernel sums in fp32, so a selection may differ from float64 where two scores are closer than the rounding of either:
eps_i = (2 tok + 128 + 4) 2^-24 max_j sum_d mean|q|[i][d] mean|k|[j][d] (an fp32 sum of tok terms, then a 128-term dot).  Every
case first asserts, from the reference alone, that the last selected and the first unselected score of every row are more than
2 eps apart (the seeds are chosen so); then the lists must be EQUAL.

One geometry: latent (10,6,8), tile (2,3,4): 20 tiles (not a multiple of 32 or of the 4 query tiles of a workgroup) of 24 rows
(not a multiple of the 16 rows of a pass)."""
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
