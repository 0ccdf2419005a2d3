"""Host: the launch dictionaries `routed_attention` hands ops.attn_fwd_batch for the sliding-tile expert, in each of its five
forms -- partial geometry, "share", "content" / "mass", the merged window and the un-merged window -- against literal
expectations: every key, the scalar values, and the tables as the very tensors the geometry caches or the selection returned.
The fused grid, `record=` (what the backward replays), the `fused_n_splits` / `fused_first` hints and the text launch all read
these dictionaries.  No GPU: the geometry's lazily built tables are small CPU tensors placed in its cache, and the launch
functions of vorta_amd.ops are recorders.  Two heads, both on expert 2; Hunyuan layout with 16 text rows, 5 of them valid."""
import pytest
import torch

LATENT, TILE, WINDOW, GROUP = (4, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)
H, D, T, TE, TOK, N_TILES = 2, 128, 16, 5, 24, 8
N_KV = N_TILES * TOK + TE  # the window holds every tile of this grid: n_sel = 8


def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def _same(a, b):
    """scalars equal; tensors the same view of the same memory"""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.data_ptr() == b.data_ptr()
                and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype)
    return type(a) is type(b) and a == b


def _assert_calls(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (i, sorted(set(g) ^ set(w)))
        for key in w:
            assert _same(g[key], w[key]), (i, key, g[key], w[key])


def _run(monkeypatch, latent=LATENT, sliding_block_rows=0, seed=None, **geom_kw):
    """(the dictionaries of the one fused grid, what the selection launches were given, geom, the expected common part and
    text launch)"""
    from vorta_amd import ops, routed
    geom = routed.RoutedGeometry(latent, TILE, WINDOW, GROUP, 0.5, torch.device("cpu"), **geom_kw)
    for key, val in (seed or {}).items():
        geom._sta[key] = val
    grids, selections = [], []
    monkeypatch.setattr(ops, "attn_fwd_batch", lambda calls: grids.append(list(calls)))
    monkeypatch.setattr(ops, "sta_tile_mass", lambda *a, **kw: selections.append(("mass", a, kw)))

    def select(*a, **kw):
        selections.append(("select", a, kw))
        return kw["out"][0], kw["out"][1], N_KV

    def share(*a, **kw):
        selections.append(("share", a, kw))
        return a[5]

    monkeypatch.setattr(ops, "sta_select_tiles", select)
    monkeypatch.setattr(ops, "sta_select_tiles_share", share)
    S = geom.S
    q, k, v = (torch.zeros((1, H, S + T, D), dtype=torch.bfloat16) for _ in range(3))
    out = torch.empty_like(q)
    routing = routed.HeadRouting.from_expert_ids([2] * H, "cpu")
    with torch.no_grad():
        routed.routed_attention(q, k, v, routing, geom, model="hunyuan", text_len=T, text_valid=TE, out=out, scale=0.25,
                                sliding_block_rows=sliding_block_rows, fp8=False)
    assert len(grids) == 1
    common = dict(q=q[0], k=k[0], v=v[0], out=out[0], scale=0.25, v_descale=None, i8=None, head_list=routing.lists[2], n_heads=H,
                  n_heads_dev=None)
    text = dict(common, n_q=T, q_valid=TE, n_kv=S + TE, n_splits=routed._auto_splits(H, T, S + TE), tag="sliding_text",
                flops=H * 4.0 * D * TE * (S + TE), q_row_offset=S)
    if routed.FUSED_TEXT_FIRST:
        text.update(fused_n_splits=routed.FUSED_TEXT_SPLITS, fused_first=True)
    return grids[0], selections, geom, common, text


def _window_tables():
    return {TE: (_i32(N_TILES * TOK), _i32(N_TILES, N_KV), N_KV)}


@pytest.mark.parametrize("block_rows", [0, 128])
def test_window_merged(monkeypatch, block_rows):
    from vorta_amd import routed
    monkeypatch.setattr(routed, "STA_MERGE", True)  # (the default; VORTA_DEBUG sta_merge=0 is an A/B switch)
    br = block_rows or 256  # (a fused call without a choice takes 256-row workgroups)
    merged = (_i32(N_TILES * TOK), _i32(1, N_KV), N_KV, _i32(1, 3), 1)
    calls, selections, geom, common, text = _run(monkeypatch, sliding_block_rows=block_rows, sliding_keys="window",
                                                 seed={**_window_tables(), ("merged", TE, br): merged})
    S = geom.S
    want = dict(common, n_q=S, n_kv=N_KV, q_rows=merged[0], kv_rows=merged[1], kv_rows_stride_g=N_KV, q_block_table=merged[3],
                n_key_lists=1, tag="sliding", flops=H * 4.0 * D * S * N_KV, block_rows=br)
    _assert_calls(calls, [want, text])
    assert not selections


def test_window_unmerged(monkeypatch):
    """a workgroup size the merged form does not take: a tile is a group, block_rows is passed on as given"""
    tables = _window_tables()
    calls, selections, geom, common, text = _run(monkeypatch, sliding_block_rows=64, sliding_keys="window", seed=tables)
    S, (q_rows, kv_rows, _) = geom.S, tables[TE]
    want = dict(common, n_q=S, q_group_len=TOK, n_kv=N_KV, q_rows=q_rows, kv_rows=kv_rows, kv_rows_stride_g=N_KV, tag="sliding",
                flops=H * 4.0 * D * S * N_KV, block_rows=64)
    _assert_calls(calls, [want, text])
    assert not selections


@pytest.mark.parametrize("keys,scores,block_rows", [("content", "mean", 64), ("mass", "mass", 0)])
def test_content_and_mass(monkeypatch, keys, scores, block_rows):
    """the lists the selection returned, a tile a group; block_rows as given (0: the fused call's 256)"""
    from vorta_amd import routed
    tables = _window_tables()
    calls, selections, geom, common, text = _run(monkeypatch, sliding_block_rows=block_rows, sliding_keys=keys, seed=tables)
    S, q_rows = geom.S, tables[TE][0]
    bufs = geom.selection_buffers(TE, H)
    assert bufs is geom.content_buffers(TE, H) and len(bufs) == 3
    want = dict(common, n_q=S, q_group_len=TOK, n_kv=N_KV, q_rows=q_rows, kv_rows=bufs[0], kv_rows_stride_g=bufs[0].stride(1),
                tag="sliding", flops=H * 4.0 * D * S * N_KV, block_rows=block_rows or 256)
    _assert_calls(calls, [want, text])
    (name, a, kw), = selections
    assert name == "select" and a[2:6] == (LATENT, TILE, WINDOW, TE) and a[6] is q_rows and kw["out"] is bufs
    assert kw["scores"] == scores and kw["scale"] == 0.25 and kw["rows_per_tile"] == routed.MASS_ROWS_PER_TILE
    assert kw["n_heads"] == H and kw["n_heads_dev"] is None and _same(kw["head_list"], common["head_list"])


@pytest.mark.parametrize("block_rows", [64, 128])
def test_share(monkeypatch, block_rows):
    """the variable-length launch: the share tables' lists, lengths and order; 128- or 256-row workgroups whatever was asked"""
    from vorta_amd import ops, routed
    br = block_rows if block_rows in (128, 256) else 256
    tables = _window_tables()
    calls, selections, geom, common, text = _run(monkeypatch, sliding_block_rows=block_rows, sliding_keys="share", mass_share=0.9,
                                                 seed=tables)
    S, q_rows = geom.S, tables[TE][0]
    tabs = geom.selection_buffers(TE, H, br)
    assert isinstance(tabs, ops.ShareTiles) and tabs is geom.share_buffers(TE, H, br)
    want = dict(common, n_q=S, q_group_len=TOK, n_kv=N_KV, q_rows=q_rows, kv_rows=tabs.kv_rows,
                kv_rows_stride_g=tabs.kv_rows.stride(1), kv_len=tabs.kv_len, order=tabs.order, tag="sliding",
                flops=H * 4.0 * D * S * N_KV, block_rows=br)
    _assert_calls(calls, [want, text])
    (n0, a0, kw0), (n1, a1, kw1) = selections
    assert n0 == "mass" and a0[6] is q_rows and a0[7] is tabs.ws and kw0["scale"] == 0.25 and kw0["n_heads"] == H
    assert n1 == "share" and a1[:4] == (LATENT, TILE, WINDOW, TE) and a1[4] is q_rows and a1[5] is tabs
    assert kw1 == dict(mass_share=0.9, n_heads=H, rows_per_tile=routed.MASS_ROWS_PER_TILE, block_rows=br, n_heads_dev=None)


def test_partial_geometry(monkeypatch):
    """one launch per key-list length, always at 128- or 256-row workgroups"""
    latent = (5, 6, 8)  # the tile's first dimension does not divide
    S = 5 * 6 * 8
    launches = [(_i32(192), _i32(2, 200), 200, 197, _i32(2, 3), 2), (_i32(48), _i32(1, 200), 200, 101, _i32(1, 3), 1)]
    calls, selections, geom, common, text = _run(monkeypatch, latent=latent, sliding_block_rows=64, partial=True,
                                                 sliding_keys="window", seed={("partial", TE, 256): launches})
    assert geom.is_partial and geom.S == S
    want = [dict(common, n_q=q_rows.numel(), n_kv=n_kv, q_rows=q_rows, kv_rows=kv_rows, kv_rows_stride_g=stride,
                 q_block_table=table, n_key_lists=n_lists, tag="sliding", flops=H * 4.0 * D * q_rows.numel() * n_kv, block_rows=256)
            for q_rows, kv_rows, stride, n_kv, table, n_lists in launches]
    _assert_calls(calls, want + [text])
    assert not selections
