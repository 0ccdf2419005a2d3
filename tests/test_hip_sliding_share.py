"""GPU: sliding_keys="share" (DESIGN.md 6.12).  The selection vorta_sta_select_tiles_share (csrc/sta_share.hip) against its
numpy restatement (tests/_share_restate.py) as integers, on score matrices written directly into ws -- every entry a multiple
of 2^-10, so every prefix sum is exact in float32, and no prefix sum equal to the threshold (asserted by the restatement): no
case rests on a rounding.  Latent (6,6,8), tile (2,3,4), window (1,3,3): 12 tiles of 24 rows, n_sel = 4; three head slots, the
device count 2.  Then `routed_attention` under "share" end to end against float64 attention over the lists the device chose,
read back, at the rule tests/test_hip_sliding_mass.py holds the mass launch to (`unit_ratios` <= 1 of tests/_attn_fwd_model.py),
on a local head and a white-noise head of the 16-tile, 12-key-tile geometry of the sliding tests; and the refusals."""
import numpy as np
import pytest
import torch

import _attn_fwd_model as F
import _random_launch as RL
import _share_restate as R
import _structured_inputs as SI
import test_hip_attention_bwd as B
from _util import dev
from test_hip_sliding_content import _geom, _routed

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, N_TILES, N_SEL, TOK, R_TILE = (6, 6, 8), (2, 3, 4), (1, 3, 3), 12, 4, 24, 16
SLOTS, LIVE, FILL = 3, 2, -7


def _scores(case):
    """(score (SLOTS, N_TILES, N_TILES) float32 in multiples of 2^-10, mass_share)"""
    rng = np.random.default_rng(3)
    shape = (SLOTS, N_TILES, N_TILES)
    if case == "ties":  # four distinct values: equal scores in every row; 0.6 * 16 is no multiple of 2^-10
        return 2.0 * rng.integers(0, 4, shape).astype(np.float32), 0.6
    if case == "nan":  # a NaN ranks first by its bits and its prefix sum never compares: that row keeps n_sel
        s = rng.integers(0, 6 << 10, shape).astype(np.float32) / 1024
        s[:, ::3, 5] = np.nan
        return s, 0.55
    if case == "every_count_1":  # the own tile alone passes 16 * 2^-10
        s = rng.integers(0, 1 << 10, shape).astype(np.float32) / 1024
        s[:, np.arange(N_TILES), np.arange(N_TILES)] += 1
        return s, 2.0 ** -10
    assert case == "mass_outside"  # p = 1 and rows whose best four tiles hold under 8 of 16: every count is n_sel
    return 1 + rng.integers(0, 1 << 10, shape).astype(np.float32) / 1024, 1.0


@pytest.mark.parametrize("t_eff", [0, 5])
@pytest.mark.parametrize("case", ["ties", "nan", "every_count_1", "mass_outside"])
def test_selection_equals_the_restatement(case, t_eff):
    from vorta_amd import ops
    score, p = _scores(case)
    q_rows, _ = ops.sta_build_tables(LATENT, TILE, WINDOW, t_eff, dev())
    n_kv = N_SEL * TOK + t_eff
    tabs = ops.sta_share_buffers(SLOTS, N_TILES, N_SEL, n_kv, dev(), R_TILE, 1)
    for x in tabs[:5]:
        x.fill_(FILL)
    tabs.ws[:score.size] = torch.as_tensor(score.reshape(-1), device=dev())
    ops.sta_select_tiles_share(LATENT, TILE, WINDOW, t_eff, q_rows, tabs, mass_share=p, n_heads=SLOTS, rows_per_tile=R_TILE,
                               block_rows=128, n_heads_dev=torch.tensor([LIVE], dtype=torch.int32, device=dev()))
    torch.cuda.synchronize()
    count, tiles, kv_len, lists = R.select_share(score[:LIVE], p, R_TILE, N_SEL, TOK, t_eff, q_rows.cpu().numpy(), strict=True)
    kv, sel, cnt, length, order, _ = (x.cpu().numpy() for x in tabs)
    assert (cnt[:LIVE] == count).all() and (sel[:LIVE] == tiles).all() and (length[:LIVE] == kv_len).all()
    for y in range(LIVE):
        for i in range(N_TILES):
            assert (kv[y, i, :kv_len[y, i]] == lists[y][i]).all(), (y, i)
    assert (cnt[LIVE:] == FILL).all() and (sel[LIVE:] == FILL).all() and (kv[LIVE:] == FILL).all(), "a dead slot was written"
    assert sorted(order.tolist()) == list(range(SLOTS * N_TILES))
    by_order = np.concatenate([count.reshape(-1), np.zeros(N_TILES * (SLOTS - LIVE), np.int32)])[order]
    assert (np.diff(by_order) <= 0).all(), "order: tile counts must not increase"
    if case == "every_count_1":
        assert (count == 1).all()
    if case == "mass_outside":
        assert (count == N_SEL).all()
        dummy = torch.zeros((SLOTS, N_TILES * TOK + t_eff, 128), dtype=torch.bfloat16, device=dev())
        fixed = ops.sta_select_buffers(SLOTS, N_TILES, N_SEL, n_kv, dev(), "mass", R_TILE)
        fixed[2][:score.size] = tabs.ws[:score.size]
        ops.sta_select_tiles(dummy, dummy, LATENT, TILE, WINDOW, t_eff, q_rows, out=fixed, phases=3, n_heads=LIVE)
        assert torch.equal(fixed[0][:LIVE], tabs.kv_rows[:LIVE]) and torch.equal(fixed[1][:LIVE], tabs.sel_tiles[:LIVE])


@pytest.mark.parametrize("t_eff", [0, 5])
def test_share_and_fixed_count_are_one_order(t_eff):
    """80 key tiles, a NaN on the diagonal of every score row: every prefix sum is NaN and never compares, so share keeps
    n_sel tiles -- the n_sel first of its rank order, which must be vorta_sta_select_tiles' (phases 3) bit for bit"""
    import test_hip_sta_select as W
    from vorta_amd import ops
    n_tiles, n_sel, tok = 80, W.WIDE_N_SEL, W.WIDE_TOK
    score = R.planted_scores(W.WIDE_SLOTS, n_tiles)
    score[:, np.arange(n_tiles), np.arange(n_tiles)] = np.nan
    q_rows, tabs = W.wide_tables(n_tiles, t_eff, score)
    kv, sel = W.wide_select(n_tiles, t_eff, q_rows, tabs)
    ops.sta_select_tiles_share(W.WIDE[n_tiles], W.WIDE_TILE, W.WIDE_WINDOW, t_eff, q_rows, tabs, mass_share=0.5,
                               n_heads=W.WIDE_SLOTS, rows_per_tile=tok, block_rows=128)
    torch.cuda.synchronize()
    assert R.straddles(sel.cpu().numpy()).all()  # (the kept tiles lie on both sides of tile 64)
    assert torch.equal(tabs.sel_tiles, sel) and torch.equal(tabs.kv_rows, kv)
    assert (tabs.sel_count == n_sel).all() and (tabs.kv_len == n_sel * tok + t_eff).all()


@pytest.mark.parametrize("dtype", F.DTYPES, ids=F.dtype_name)
def test_share_launch_against_float64_over_the_lists_it_chose(dtype):
    """head 0 local (its mass on a few tiles: 4 to 7 of 12 kept at p = 0.9 by the restatement on the float64 statistic), head 1
    white noise (a flat row: all 12 kept)"""
    gen = torch.Generator(device="cpu").manual_seed(5)
    local = SI.local_head(B.LATENT, (2.0, 3.0, 4.0), 8.0, 0.2, gen, "cpu")
    white = tuple(torch.randn((B.S_VID, 128), generator=gen) for _ in range(3))
    q, k, v = (torch.stack([a, b])[None].to(dtype).to(dev()) for a, b in zip(local, white))
    geom = _geom(sliding_keys="share", mass_share=0.9)
    out = torch.full_like(q, RL.SENTINEL)
    _routed(q, k, v, geom, "wan", 0, 0, out=out, fp8=False)
    torch.cuda.synchronize()
    tabs, q_rows = geom.share_buffers(0, 2, 256), geom.sta_tables(0)[0]
    n_sel, count = tabs.sel_tiles.shape[2], tabs.sel_count.cpu()
    print(f"kept tiles per head: mean {count.float().mean(1).tolist()}, min {int(count.min())}, max {int(count.max())} of {n_sel}")
    assert int(count.min()) < n_sel and int(count.max()) == n_sel, "the variable path needs short AND full lists"
    assert torch.equal(tabs.kv_len.cpu(), count * geom.tok)
    kws = [dict(n_q=geom.tok, q_rows=q_rows[i * geom.tok:(i + 1) * geom.tok], n_kv=int(tabs.kv_len[y, i]),
                kv_rows=tabs.kv_rows[y, i, :int(tabs.kv_len[y, i])], head_list=torch.tensor([y], dtype=torch.int32), n_heads=1)
           for y in range(2) for i in range(tabs.kv_len.shape[1])]
    ref = lambda **o: sum(F.model_out(kw, q[0], k[0], v[0], dtype, **o) for kw in kws)  # noqa: E731  (disjoint rows, fill 0)
    c = dict(f64=ref(round16=False), model=ref(), f32=ref(round16=False, work=torch.float32),
             valid=torch.ones((2, B.S_VID), dtype=torch.bool))
    for unit, x in F.unit_ratios(out[0].cpu(), c).items():
        print(f"{F.dtype_name(dtype)} {unit}: e_hip / bound max {float(x.max()):.3f}")
        assert float(x.max()) <= 1.0, (unit, float(x.max()))


def test_share_is_refused_by_name_where_it_does_not_run(monkeypatch):
    from test_hip_patch_sampled_expert_fidelity import _setup
    from vorta.patch import measured_routes
    from vorta_amd import routed
    monkeypatch.delenv("VORTA_SLIDING_MASS_SHARE", raising=False)
    with pytest.raises(ValueError, match="'share' has no default share"):
        _geom(sliding_keys="share")
    with pytest.raises(ValueError, match="sliding_keys='share' on a partial geometry"):
        routed.RoutedGeometry((9, 6, 8), B.TILE, B.WINDOW, B.GROUP, 0.5, dev(), partial=True, sliding_keys="share", mass_share=0.9)
    with pytest.raises(ValueError, match="sliding_keys='share' under sequence parallelism"):
        _geom(sliding_keys="share", mass_share=0.9, row_map=torch.arange(B.S_VID, dtype=torch.int32, device=dev()))
    geom = _geom(sliding_keys="share", mass_share=0.9)
    q, k, v = (torch.randn((1, 2, B.S_VID, 128), device=dev()).bfloat16() for _ in range(3))
    for fn, kw in ((routed.sampled_expert_fidelity, {}), (routed.route_by_fidelity, dict(max_rel_error=0.1))):
        with pytest.raises(ValueError, match=f"{fn.__name__}: sliding_keys='share'.*per-head sampled form"):
            fn(q, k, v, geom, model="wan", **kw)
    with pytest.raises(ValueError, match="sliding_keys='share' in grad mode"):
        _routed(q.requires_grad_(True), k, v, geom, "wan", 0, 0)
    with pytest.raises(ValueError, match="sliding_keys='share' in grad mode"):
        _routed(q.detach(), k, v, geom, "wan", 0, 0, record=[])
    monkeypatch.setattr(routed, "_sliding_keys", "share")
    monkeypatch.setattr(routed, "_mass_share", 0.9)
    with pytest.raises(ValueError, match="measured_routes: sliding_keys='share'.*per-head sampled form"):
        with measured_routes(_setup("wan")[0], max_rel_error=0.1):
            pass
