"""GPU: vorta_sta_tile_mass (csrc/sta_mass.hip) and the selection from its matrix (vorta_sta_select_tiles, phases 3) against the
rule in float64 on the same 16-bit inputs: r sampled rows x of query tile i (positions i tok + floor((2s+1) tok / (2r))),
l = scale <q_x, k_p> over every video key p, p_x(j) = sum_{p in tile j} exp(l) / sum_p exp(l), score[i][j] = sum_s p_x(j); then
tile i itself and the n_sel - 1 tiles j != i of highest score, ties to the lower j, ascending, expanded through q_rows.

The bound on a score, from the kernels' arithmetic (u = 2^-24, G_x = max_p sum_d |q_x||k_p|, cpt = ceil(tok / 64) staged chunks a
tile): a logit is off by at most e_x = (128 + 2) u scale G_x (128 fp32 products accumulated, the scale multiply, the fused
subtraction of the running max) and the reduction subtracts two maxima once more, + 2 u scale G_x; numerator and denominator of
p_x(j) each move by at most exp(e_x): expm1(2 e_x).  The hardware exp2 is good to 1 ulp = 2u and a term passes through at most
cpt + 2 of them (its own, a rescale per chunk, the reduction's), in numerator and denominator: 4 (cpt + 2) u.  The fp32 sums: a
term passes at most tok + cpt + 1 additions inside its tile and n_tiles across tiles, cpt + 1 multiplications and one division,
again on both sides: (2 (tok + n_tiles) + 4 cpt + 8) u.  The sum over the r rows adds r u score.  So
eps[i][j] = sum_s p_x(j) rel_x + r u score[i][j],  rel_x = expm1(2 e_x) + (2 (tok + n_tiles) + 8 cpt + 16) u.
Every case first asserts, from the reference alone, that the last selected and the first unselected score of every row are more
than twice their eps apart (q and k are scaled by 3 so that the masses are peaked, and the seeds are chosen so; checked on the
CPU); then the scores lie within eps and the lists are EQUAL.

Latent (10,6,8).  Tile (2,3,4): 20 tiles of 24 rows -- a key tile shorter than one 32-key block, 20 not a multiple of the query
tiles of a wave (2 or 4) or of a workgroup.  Tile (2,3,8): 10 tiles of 48 rows -- one full and one masked block a tile."""
import pytest
import torch

from _util import dev

pytestmark = pytest.mark.gpu

LATENT, S, H, SCALE, FILL = (10, 6, 8), 480, 3, 128 ** -0.5, -7
N_ROWS = S + 5 + 11  # rows of q and k: video, text and rows only a row_map reaches
# tok -> (tile, n_sel -> window: the own tile only, an interior count, every tile; 2: the planted case's)
GEOMETRY = {24: ((2, 3, 4), {1: (1, 1, 1), 2: (1, 3, 1), 6: (3, 3, 1), 20: (5, 3, 3)}),
            48: ((2, 3, 8), {1: (1, 1, 1), 3: (3, 1, 1), 10: (5, 3, 1)})}
INTERIOR = {24: 6, 48: 3}


def _reference(q, k, q_rows, tok, r, n_sel, heads):
    """(score (slots, n_tiles, n_tiles) float64, its eps, sel_tiles (slots, n_tiles, n_sel)); asserts the near-tie precondition"""
    nt, u, cpt = S // tok, 2.0 ** -24, (tok + 63) // 64
    rows = q_rows.cpu().long()
    pos = (torch.arange(nt)[:, None] * tok + ((2 * torch.arange(r) + 1) * tok) // (2 * r)).flatten()
    qs, kt = q.double().cpu()[heads][:, rows[pos]], k.double().cpu()[heads][:, rows]
    p = torch.softmax(SCALE * qs @ kt.transpose(1, 2), -1).view(len(heads), nt, r, nt, tok).sum(-1)
    G = (qs.abs() @ kt.abs().transpose(1, 2)).amax(-1).view(len(heads), nt, r)
    rel = torch.expm1(2 * (128 + 2 + 2) * u * SCALE * G) + (2 * (tok + nt) + 8 * cpt + 16) * u
    score = p.sum(2)
    eps = (p * rel[..., None]).sum(2) + r * u * score
    ranked, own = score.clone(), torch.arange(nt)
    ranked[:, own, own] = float("inf")  # the tile itself is always selected
    order = torch.argsort(ranked, dim=-1, descending=True, stable=True)  # (stable: equal scores go to the lower j)
    if 1 < n_sel < nt:
        a, b = order[..., n_sel - 1:n_sel], order[..., n_sel:n_sel + 1]
        gap = (score.gather(-1, a) - score.gather(-1, b)) / (2 * torch.maximum(eps.gather(-1, a), eps.gather(-1, b)))
        assert (gap > 1).all(), f"near tie: gap / 2 eps min {float(gap.min()):.2f} (choose another seed)"
    return score, eps, order[..., :n_sel].sort(-1).values.to(torch.int32)


def _inputs(dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple((3.0 * torch.randn((H, N_ROWS, 128), generator=gen)).to(dtype) for _ in range(2))


def _run(q, k, tok, r, n_sel, t_eff, row_map=None, head_list=None, n_heads_dev=None):
    from vorta_amd import ops
    tile, windows = GEOMETRY[tok]
    window, nt = windows[n_sel], S // tok
    q, k = q.to(dev()), k.to(dev())
    q_rows, _ = ops.sta_build_tables(LATENT, tile, window, t_eff, dev(), row_map=row_map)
    n_slots = H if head_list is None else head_list.numel()
    bufs = ops.sta_select_buffers(n_slots, nt, n_sel, n_sel * tok + t_eff, dev(), scores="mass", rows_per_tile=r)
    for b in bufs:
        b.fill_(FILL)
    kv, sel, n_kv = ops.sta_select_tiles(q, k, LATENT, tile, window, t_eff, q_rows, head_list=head_list, n_heads_dev=n_heads_dev,
                                         row_map=row_map, out=bufs, scores="mass", scale=SCALE, rows_per_tile=r)
    torch.cuda.synchronize()
    assert n_kv == n_sel * tok + t_eff and tuple(kv.shape) == (n_slots, nt, n_kv)
    live = n_slots if n_heads_dev is None else int(n_heads_dev.item())
    heads = list(range(H)) if head_list is None else head_list.tolist()
    score, eps, want = _reference(q, k, q_rows, tok, r, n_sel, heads[:live])
    got = bufs[2][:n_slots * nt * nt].view(n_slots, nt, nt).cpu()
    ratio = (got[:live].double() - score).abs() / eps
    print(f"tok {tok} r {r}: |score - float64| / eps max {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0
    assert torch.equal(sel[:live].cpu(), want), "sel_tiles differs from the float64 rule"
    video = q_rows.cpu().view(nt, tok)[want.long()].reshape(live, nt, n_sel * tok)
    text = torch.arange(S, S + t_eff, dtype=torch.int32)
    if row_map is not None:
        text = row_map.cpu()[text.long()]
    assert torch.equal(kv[:live].cpu(), torch.cat([video, text.expand(live, nt, t_eff)], dim=-1))
    assert (kv[live:] == FILL).all() and (sel[live:] == FILL).all() and (got[live:] == FILL).all(), \
        "slots past the device count were written"
    return want


# (seed: the first for which the precondition of _reference holds at the interior count of every tile size)
@pytest.mark.parametrize("t_eff", [0, 5])
@pytest.mark.parametrize("which", ["own", "interior", "all"])
@pytest.mark.parametrize("r", [8, 16])
@pytest.mark.parametrize("tok", [24, 48])
@pytest.mark.parametrize("dtype,seed", [(torch.bfloat16, 2), (torch.float16, 1)], ids=["bf16", "fp16"])
def test_scores_and_selection_match_float64(dtype, seed, tok, r, which, t_eff):
    q, k = _inputs(dtype, seed)
    _run(q, k, tok, r, {"own": 1, "interior": INTERIOR[tok], "all": S // tok}[which], t_eff)


def test_head_list_with_a_device_count_leaves_trailing_slots_alone():
    q, k = _inputs(torch.bfloat16, 2)
    _run(q, k, 24, 16, 6, 5, head_list=torch.tensor([2, 0, 1], dtype=torch.int32, device=dev()),
         n_heads_dev=torch.tensor([2], dtype=torch.int32, device=dev()))


def test_row_map():
    """token i lives in physical row row_map[i] of q and k (a permutation into a longer buffer): the sampled rows and the keys
    follow q_rows, the lists hold physical rows, the text rows included"""
    row_map = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(4))[:S + 5].to(torch.int32).to(dev())
    q, k = _inputs(torch.float16, 2)
    _run(q, k, 48, 8, 3, 5, row_map=row_map)


def test_planted_far_tile_no_mean_can_find():
    """the rows of key tile j are +-8 along axis j (alternating, over small noise) and the rows of query tile i are EXACTLY +-8
    along the axis of a far tile far(i) >= 10: every row of tile i points at tile far(i), and the tile's mean q is zero.  The
    mass rule selects far(i); the mean rule, restated in float64, scores every tile 0 and takes the lowest one (n_sel = 2: the tile itself and one other)"""
    tok, nt = 24, 20
    from vorta_amd import ops
    pos, far = torch.arange(S), 10 + torch.arange(nt) % 9  # (far(i) != i)
    rows = ops.sta_build_tables(LATENT, GEOMETRY[tok][0], GEOMETRY[tok][1][2], 0, dev())[0].cpu().long()
    sign = (1.0 - 2.0 * (pos % 2))[:, None]
    q, k = (0.05 * x.float() / 3.0 for x in _inputs(torch.bfloat16, 0))
    q[:, rows] = 8.0 * sign * torch.nn.functional.one_hot(far[pos // tok], 128)
    k[:, rows] += 8.0 * sign * torch.nn.functional.one_hot(pos // tok, 128)
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    want = _run(q, k, tok, 16, 2, 0)
    assert (want == far.to(torch.int32)[None, :, None]).any(-1).all(), "the mass rule misses the planted tile"
    mean = q.double()[:, rows].view(H, nt, tok, 128).mean(2) @ k.double()[:, rows].view(H, nt, tok, 128).mean(2).transpose(1, 2)
    assert not mean.any(), "the planted tiles' mean q is not zero"
    mean[:, torch.arange(nt), torch.arange(nt)] = float("inf")
    by_mean = torch.argsort(mean, dim=-1, descending=True, stable=True)[..., :2]
    assert not (by_mean == far[None, :, None]).any(), "the mean rule found the planted tile"
