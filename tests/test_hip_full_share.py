"""GPU: the full-attention expert on the fewest key tiles holding a mass share (full_keys="share"): the selection over ALL
tiles (csrc/sta_share_all.hip) against the numpy restatement, the tile-list launch (csrc/attn_fwd_tilelist.hip) bit for bit
against the row-table launch on the same lists expanded, and both through routed_attention.

Shape A: latent (8,6,8), tile (2,3,4): tok = 24, 16 tiles -- a 64-key block straddles 3-4 tiles.  Shape B: tile (4,3,8): tok = 96,
4 tiles -- a tile spans blocks.  3 head slots behind the head list (2, 0, 1), device count 2: the third slot stays untouched."""
import functools

import numpy as np
import pytest
import torch

import _share_restate as R
from _util import ATOL_SAME, dev, rounded, to_dev

pytestmark = pytest.mark.gpu

LATENT, WINDOW, S, T, SENTINEL = (8, 6, 8), (3, 3, 3), 384, 16, 7.0
TILES = {"A": (2, 3, 4), "B": (4, 3, 8)}
HEADS, SLOTS, LIVE = [2, 0, 1], 3, 2
t = lambda a: torch.as_tensor(np.asarray(a), device=dev())  # noqa: E731


def _attention(q, k, v, keys):
    z = q @ k[keys].T / np.sqrt(128.0)
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ v[keys]


# ---- 1. the selection ----
@pytest.mark.parametrize("p", [0.05, 0.3])
def test_selection_over_all_tiles_matches_the_restatement(p):
    from vorta_amd import ops
    latent, tile, r = (10, 8, 8), (1, 2, 4), 8  # 80 tiles of 8 rows: two 64-lane passes of the rank and of the list
    n_tiles, tok, t_eff = 80, 8, 11
    score = R.planted_scores(SLOTS, n_tiles)
    tabs = ops.sta_share_all_buffers(SLOTS, n_tiles, dev(), r, 1)
    for x in tabs[:4]:
        x.fill_(-7)
    tabs.ws[:score.size] = t(score).reshape(-1)
    ops.sta_select_tiles_share_all(latent, tile, t_eff, tabs, mass_share=p, n_heads=SLOTS, rows_per_tile=r, block_rows=128,
                                   n_heads_dev=t(np.array([LIVE], np.int32)))
    count, tiles, kv_len, _ = R.select_share(score[:LIVE], p, r, n_tiles, tok, t_eff, np.arange(n_tiles * tok))
    got_c, got_t, got_l, order = (x.cpu().numpy() for x in (tabs.sel_count, tabs.sel_tiles, tabs.kv_len, tabs.order))
    assert (got_c[:LIVE] == count).all() and (got_t[:LIVE] == tiles).all() and (got_l[:LIVE] == kv_len).all()
    assert count[0, 1] == n_tiles, "a NaN score sums to NaN: every tile is kept"
    assert count.min() < 64 < count.max()  # short lists, and lists past the first 64-lane pass
    assert (got_c[LIVE:] == -7).all() and (got_t[LIVE:] == -7).all() and (got_l[LIVE:] == -7).all()
    per_item = np.concatenate([count.reshape(-1), np.zeros(n_tiles, np.int32)])  # blocks_per_group = 1; the dead slot counts 0
    assert sorted(order.tolist()) == list(range(SLOTS * n_tiles))
    assert (order == np.argsort(-per_item, kind="stable")).all()


def test_share_one_keeps_every_tile():
    from vorta_amd import ops
    tabs = ops.sta_share_all_buffers(1, 16, dev(), 16, 1)
    tabs.ws[:256] = 1.0  # a row of 16 tiles sums to rows_per_tile = 16 at its LAST tile, exactly
    ops.sta_select_tiles_share_all(LATENT, TILES["A"], 11, tabs, mass_share=1.0, n_heads=1, rows_per_tile=16)
    assert (tabs.sel_count.cpu() == 16).all() and (tabs.sel_tiles.cpu() == torch.arange(16, dtype=torch.int32)).all()
    assert (tabs.kv_len.cpu() == 16 * 24 + 11).all()


# ---- 2. the launch ----
@functools.lru_cache(maxsize=None)
def _launch_case(shape, t_eff):
    """q, k, v (a last row of NaN that no list names), hand-made tile lists -- one tile, every tile, and counts whose video
    part ends inside a key block, in one launch --, the same lists expanded into rows, and q_valid"""
    tile = TILES[shape]
    tok = tile[0] * tile[1] * tile[2]
    n_tiles = S // tok
    rng = np.random.default_rng(5)
    q, k, v = (rng.standard_normal((SLOTS, S + T + 1, 128)) for _ in range(3))
    k[:, -1], v[:, -1] = np.nan, np.nan
    counts = np.array([1, n_tiles, 3, max(n_tiles // 2, 1), n_tiles - 1, 2] * 3, np.int32)
    count = np.stack([np.roll(counts, y)[:n_tiles] for y in range(SLOTS)])
    tiles = np.full((SLOTS, n_tiles, n_tiles), -1, np.int32)
    for y in range(SLOTS):
        for g in range(n_tiles):
            tiles[y, g, :count[y, g]] = np.sort(rng.permutation(n_tiles)[:count[y, g]])
    return q, k, v, tiles, count, tok, n_tiles, S - 30


def _expanded(case, t_eff, q_rows):
    _, _, _, tiles, count, tok, n_tiles, _ = case
    n_kv = n_tiles * tok + t_eff
    kv = np.full((SLOTS, n_tiles, n_kv), S + T, np.int32)  # (the NaN row behind every list)
    for y in range(SLOTS):
        for g in range(n_tiles):
            rows = q_rows.reshape(n_tiles, tok)[tiles[y, g, :count[y, g]]].reshape(-1)
            kv[y, g, :rows.size + t_eff] = np.concatenate([rows, np.arange(S, S + t_eff)])
    return kv, (count * tok + t_eff).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _launch_reference(shape, t_eff, dtype):
    case = _launch_case(shape, t_eff)
    q, k, v, tiles, count, tok, n_tiles, q_valid = case
    from vorta_amd import ops
    q_rows = ops.sta_build_tables(LATENT, TILES[shape], WINDOW, t_eff, dev())[0].cpu().numpy()
    kv, kv_len = _expanded(case, t_eff, q_rows)
    rq, rk, rv = (rounded(x, dtype) for x in (q, k, v))
    ref = np.full(q.shape, SENTINEL)
    for y in range(LIVE):
        h = HEADS[y]
        ref[h, q_rows] = 0.0
        for g in range(n_tiles):
            rows = q_rows[g * tok:min((g + 1) * tok, q_valid)]
            if rows.size:
                ref[h, rows] = _attention(rq[h, rows], rk[h], rv[h], kv[y, g, :kv_len[y, g]])
    return ref, q_rows, kv, kv_len


@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("t_eff", [0, 11])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_tile_list_launch_writes_the_bits_of_the_row_table_launch(shape, t_eff, dtype, block_rows):
    from vorta_amd import ops
    q, k, v, tiles, count, tok, n_tiles, q_valid = _launch_case(shape, t_eff)
    ref, q_rows, kv, kv_len = _launch_reference(shape, t_eff, dtype)
    qd, kd, vd = (to_dev(x, dtype) for x in (q, k, v))
    n_wg = SLOTS * n_tiles * -(-tok // block_rows)
    order = torch.arange(n_wg - 1, -1, -1, dtype=torch.int32, device=dev()) if block_rows == 128 else None
    kw = dict(n_q=S, q_group_len=tok, n_kv=n_tiles * tok + t_eff, q_rows=t(q_rows), q_valid=q_valid, order=order,
              head_list=t(np.array(HEADS, np.int32)), n_heads=SLOTS, n_heads_dev=t(np.array([LIVE], np.int32)), block_rows=block_rows)
    out, out_rows = torch.full_like(qd, SENTINEL), torch.full_like(qd, SENTINEL)
    ops.attn_fwd_tilelist(qd, kd, vd, out, tile_lists=ops.TileLists(t(q_rows), t(tiles), t(count), tok), **kw)
    kvd = t(kv)
    ops.attn_fwd_varlen(qd, kd, vd, out_rows, kv_len=t(kv_len), kv_rows=kvd, kv_rows_stride_g=kvd.stride(1), **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, out_rows), "one body, two addressings: the same bits"
    got = out.float().cpu().numpy()
    assert not np.isnan(got).any(), "a row behind a list's length was read"
    err = np.abs(got - ref).max()
    print(f"max |d| {err:.3e} (bound {ATOL_SAME[dtype]})")
    assert err <= ATOL_SAME[dtype]
    assert (got[HEADS[0]][q_rows[q_valid:]] == 0).all()


# ---- 3. through routed_attention ----
EXPERTS = [0, 1, 2, 0, 1, 2]


@functools.lru_cache(maxsize=None)
def _routed_case(shape, p):
    """(q, k, v on the device, the full_keys="all" output, the "share" output, the tile lists the share call selected)"""
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention
    gen = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn((1, 6, S + T, 128), generator=gen) for _ in range(3))
    # peaked rows of moderate logits, so that a share below 1 drops tiles: the keys at half scale (logit noise of std 0.5), and
    # the rows of tile i share channel i in q and k at the size that adds 3 to the logit of a key in the query's own tile
    from vorta_amd import ops
    tok = TILES[shape][0] * TILES[shape][1] * TILES[shape][2]
    tile_of = torch.empty(S, dtype=torch.long)
    tile_of[ops.sta_build_tables(LATENT, TILES[shape], WINDOW, 11, dev())[0].cpu().long()] = torch.arange(S) // tok
    k[:, :, :S] *= 0.5
    for x in (q, k):
        x[0, :, torch.arange(S), tile_of] += (3.0 * 128 ** 0.5) ** 0.5
    q, k, v = (x.to(torch.bfloat16).to(dev()) for x in (q, k, v))
    outs = {}
    for keys in ("all", "share"):
        geom = RoutedGeometry(LATENT, TILES[shape], WINDOW, (2, 3, 2), 0.5, dev(), full_keys=keys,
                              full_mass_share=p if keys == "share" else None)
        outs[keys] = routed_attention(q, k, v, HeadRouting.from_expert_ids(EXPERTS, dev()), geom, model="hunyuan", text_len=T,
                                      text_valid=11)
    tabs = geom.full_share_buffers(2)
    torch.cuda.synchronize()
    return q, k, v, outs["all"], outs["share"], tabs.sel_tiles.cpu().numpy(), tabs.sel_count.cpu().numpy(), geom


@pytest.mark.parametrize("shape,p", [("A", 0.9), ("B", 0.9), ("A", 1.0)])
def test_routed_share_heads_attend_the_tiles_the_call_selected(shape, p):
    q, k, v, out_all, out_share, tiles, count, geom = _routed_case(shape, p)
    tok, te = geom.tok, 11
    q_rows = geom.sta_tables(te)[0].cpu().numpy()
    full, others = [0, 3], [1, 2, 4, 5]
    assert torch.equal(out_share[0, others], out_all[0, others]) and torch.equal(out_share[0, full, S:], out_all[0, full, S:])
    rq, rk, rv = (x[0].double().cpu().numpy() for x in (q, k, v))
    for y, h in enumerate(full):
        ref = np.zeros((S, 128))
        for g in range(S // tok):
            keys = np.concatenate([q_rows.reshape(-1, tok)[tiles[y, g, :count[y, g]]].reshape(-1), np.arange(S, S + te)])
            assert g in tiles[y, g, :count[y, g]], "the query tile itself comes first"
            rows = q_rows[g * tok:(g + 1) * tok]
            ref[rows] = _attention(rq[h, rows], rk[h], rv[h], keys)
        err = np.abs(out_share[0, h, :S].float().cpu().numpy() - ref).max()
        print(f"head {h}: kept {count[y].mean():.1f} of {S // tok} tiles, max |d| {err:.3e}")
        assert err <= ATOL_SAME[torch.bfloat16]
    if p == 1.0:
        assert (out_share[0, full].float() - out_all[0, full].float()).abs().max() <= ATOL_SAME[torch.bfloat16]
    else:
        assert count.min() < S // tok, "the case drops no tile: it would not tell the share launch from the dense one"


def test_repaired_heads_are_dense_under_full_keys_share():
    from vorta_amd.routed import HeadRouting, routed_attention_repaired
    q, k, v, out_all, _, _, _, geom = _routed_case("A", 0.9)
    from vorta_amd import ops
    ids = torch.tensor(EXPERTS, dtype=torch.int32, device=dev())
    host = HeadRouting.from_expert_ids(EXPERTS, dev())
    routes = HeadRouting.from_device(host.lists, torch.tensor(host.counts_host, dtype=torch.int32, device=dev())), ids
    out, rec = routed_attention_repaired(q, k, v, routes, geom, repair_above=0.0, model="hunyuan", text_len=T, text_valid=11)
    want = torch.empty_like(q)  # dense attention over every key, as full_keys="all" launches expert 0
    ops.attn_fwd(q[0], k[0], v[0], want[0], n_q=S + T, n_kv=S + 11, q_valid=S + 11)
    repaired = (rec.state_of_head == 2).nonzero().flatten().tolist()
    assert repaired == [1, 2, 4, 5]  # (a bound of 0: every checked head)
    assert torch.equal(out[0, repaired], want[0, repaired])
    # the tables hold every head under expert 0 now, which is the share launch here: in later calls with these tables -- launched
    # as they stand, or verified again -- the repaired heads are still dense, and the heads that were on expert 0 still share
    assert rec.routes.expert_ids.tolist() == [0] * 6
    for bound in (None, 0.0):
        again, rec2 = routed_attention_repaired(q, k, v, routes, geom, repair_above=bound, model="hunyuan", text_len=T, text_valid=11,
                                                out=torch.zeros_like(q))
        assert torch.equal(again[0, repaired], want[0, repaired]), bound
        assert torch.equal(again[0, [0, 3]], out[0, [0, 3]]) and not torch.equal(again[0, [0, 3], :S], want[0, [0, 3], :S])
        assert rec2 is None or int(rec2.repair_count) == 0


def test_measured_routes_refuses_full_keys_share(monkeypatch):
    from test_hip_patch_sampled_expert_fidelity import _setup
    from vorta.patch import measured_routes
    from vorta_amd import routed
    monkeypatch.setattr(routed, "_full_keys", "share")
    monkeypatch.setattr(routed, "_full_mass_share", 0.9)
    with pytest.raises(ValueError, match="measured_routes: full_keys='share'.*sampled form of the share-kept full expert is missing"):
        with measured_routes(_setup("wan")[0], max_rel_error=0.1):
            pass
