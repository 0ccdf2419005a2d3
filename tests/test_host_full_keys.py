"""Host: the `full_keys` switch -- keyword, then `set_full_keys`, then VORTA_FULL_KEYS, then "all" --, unknown names, the missing
share, the refusals of full_keys="share" by name before any launch, and the codes of the two C entry points on fake pointers."""
import ctypes

import pytest
import torch

GEOMETRY = ((8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2), 0.5, torch.device("cpu"))


@pytest.fixture(autouse=True)
def _unset(monkeypatch):
    from vorta_amd import routed
    monkeypatch.setattr(routed, "_full_keys", None)
    monkeypatch.setattr(routed, "_full_mass_share", None)
    monkeypatch.delenv("VORTA_FULL_KEYS", raising=False)
    monkeypatch.delenv("VORTA_FULL_MASS_SHARE", raising=False)


def test_precedence_keyword_then_setter_then_environment(monkeypatch):
    import vorta_amd
    from vorta_amd import routed
    g = routed.RoutedGeometry(*GEOMETRY)
    assert (g.full_keys, g.full_mass_share) == ("all", None)
    monkeypatch.setenv("VORTA_FULL_KEYS", "share")
    with pytest.raises(ValueError, match="full_keys='share' has no default share"):
        routed.RoutedGeometry(*GEOMETRY)
    monkeypatch.setenv("VORTA_FULL_MASS_SHARE", "0.9")
    g = routed.RoutedGeometry(*GEOMETRY)
    assert (g.full_keys, g.full_mass_share) == ("share", 0.9)
    vorta_amd.set_full_keys("all")  # the setter overrides the environment
    assert routed.RoutedGeometry(*GEOMETRY).full_keys == "all"
    vorta_amd.set_full_keys("share", mass_share=0.95)
    assert routed.RoutedGeometry(*GEOMETRY).full_mass_share == 0.95
    g = routed.RoutedGeometry(*GEOMETRY, full_keys="share", full_mass_share=0.5)  # the keyword overrides both
    assert (g.full_keys, g.full_mass_share, g.sliding_keys) == ("share", 0.5, "window")
    a, b = (routed.geometry_for(*GEOMETRY, full_keys=name) for name in ("all", "share"))
    assert a is not b and b is routed.geometry_for(*GEOMETRY) and a.full_keys == "all"


@pytest.mark.parametrize("how", ["keyword", "setter", "environment"])
def test_unknown_names_and_bad_shares_are_errors(how, monkeypatch):
    from vorta_amd import routed
    with pytest.raises(ValueError, match="unknown full keys 'half'.*all, share"):
        if how == "keyword":
            routed.RoutedGeometry(*GEOMETRY, full_keys="half")
        elif how == "setter":
            routed.set_full_keys("half")
        else:
            monkeypatch.setenv("VORTA_FULL_KEYS", "half")
            routed.RoutedGeometry(*GEOMETRY)
    with pytest.raises(ValueError, match="outside \\(0, 1\\]"):
        routed.RoutedGeometry(*GEOMETRY, full_keys="share", full_mass_share=1.5)
    with pytest.raises(ValueError, match="goes with 'share'"):
        routed.set_full_keys("all", mass_share=0.9)


def test_share_refuses_by_name_before_any_launch():
    """(CPU tensors throughout: a launch would fail on them, so every refusal below comes before one)"""
    from vorta_amd import routed
    from vorta_amd.routed import HeadRouting, RoutedGeometry
    share = dict(full_keys="share", full_mass_share=0.9)
    with pytest.raises(ValueError, match="full_keys='share' on a partial geometry"):
        RoutedGeometry((9, 6, 8), *GEOMETRY[1:], partial=True, **share)
    with pytest.raises(ValueError, match="full_keys='share' under sequence parallelism"):
        RoutedGeometry(*GEOMETRY, row_map=torch.arange(8 * 6 * 8, dtype=torch.int32), **share)
    geom = RoutedGeometry(*GEOMETRY, **share)
    q = torch.zeros((1, 3, 384, 128), dtype=torch.bfloat16)
    kw = dict(model="wan")
    routing = HeadRouting.from_expert_ids([0, 1, 2], q.device)
    with pytest.raises(ValueError, match="full_keys='share' in grad mode"):
        routed.routed_attention(q.clone().requires_grad_(), q, q, routing, geom, **kw)
    with pytest.raises(ValueError, match="full_keys='share' in the soft-mixture operators"):
        routed.soft_mixture_attention(q, q, q, torch.zeros((1, 3, 3)), geom, **kw)
    for precision in ("fp8pv", "i8pv", "auto8"):
        with pytest.raises(ValueError, match=f"full_keys='share' under the 8-bit precision '{precision}'.*no int8-score or e4m3 tile-list body"):
            routed.routed_attention(q, q, q, routing, geom, fp8=precision, **kw)
    with pytest.raises(ValueError, match="routed_attention\\(expert_fidelity=\\): full_keys='share'"):
        routed.routed_attention(q, q, q, routing, geom, expert_fidelity=[], **kw)
    with pytest.raises(ValueError, match="sampled_expert_fidelity: full_keys='share'"):
        routed.sampled_expert_fidelity(q, q, q, geom, **kw)
    with pytest.raises(ValueError, match="route_by_fidelity: full_keys='share'"):
        routed.route_by_fidelity(q, q, q, geom, max_rel_error=0.1, **kw)


def test_entry_points_refuse_before_any_launch():
    """Fake 4- and 16-byte-aligned pointers, never dereferenced: every call returns before a launch (no GPU needed)."""
    from vorta_amd import _C
    lib = _C.lib()
    P = 1 << 20
    EINVAL, EUNSUP = _C.VORTA_EINVAL, _C.VORTA_EUNSUPPORTED

    def attn(**kw):
        a = _C.AttnArgs()
        a.struct_size, a.head_dim, a.n_heads, a.dtype = ctypes.sizeof(_C.AttnArgs), 128, 1, _C.VORTA_BF16
        for x in (a.q, a.k, a.v, a.o):
            x.ptr, x.stride_s, x.stride_h = P, 128, 128 * 4096
        a.n_q, a.n_kv, a.q_valid, a.q_group_len, a.scale, a.block_rows, a.n_splits = 384, 384 + 11, 384, 24, 0.1, 128, 1
        for key, val in kw.items():
            setattr(a, key, val)
        return a

    def ext(**kw):
        e = _C.AttnTilelistExt()
        e.struct_size, e.tok, e.n_tiles, e.S, e.t_eff = ctypes.sizeof(_C.AttnTilelistExt), 24, 16, 384, 11
        e.tile_rows, e.tiles, e.tiles_stride_h, e.count, e.count_stride_h = P, P, 256, P, 16
        for key, val in kw.items():
            setattr(e, key, val)
        return e

    def fwd(a, e):
        return lib.vorta_attn_fwd_tilelist(ctypes.byref(a), ctypes.byref(e), None)

    for bad in (dict(n_splits=2, ws_o=P, ws_ml=P), dict(dup_rows=P), dict(variant=1), dict(dtype=_C.VORTA_FP8E4M3)):
        assert fwd(attn(**bad), ext()) == EUNSUP, bad
    assert fwd(attn(), ext(n_tiles=2048, tiles_stride_h=1 << 20)) == EUNSUP
    for bad in (dict(struct_size=8), dict(tiles=None), dict(tile_rows=None), dict(count=None), dict(tiles=P + 2), dict(order=P + 1),
                dict(tiles_stride_h=255), dict(count_stride_h=15), dict(t_eff=12), dict(tok=0)):
        assert fwd(attn(), ext(**bad)) == EINVAL, bad
    assert fwd(attn(kv_rows=P), ext()) == EINVAL

    def sel(**kw):
        s = _C.StaShareAllArgs()
        s.struct_size, s.n_heads, s.t_eff, s.rows_per_tile, s.mass_share, s.blocks_per_group = ctypes.sizeof(s), 2, 11, 16, 0.9, 1
        s.latent, s.tile = (ctypes.c_int32 * 3)(8, 6, 8), (ctypes.c_int32 * 3)(2, 3, 4)
        s.sel_count, s.sel_tiles, s.kv_len, s.ws = P, P, P, P
        for key, val in kw.items():
            setattr(s, key, val)
        return lib.vorta_sta_select_tiles_share_all(ctypes.byref(s), None)

    for bad in (dict(struct_size=8), dict(mass_share=0.0), dict(mass_share=float("nan")), dict(rows_per_tile=12), dict(ws=None),
                dict(ws=P + 4), dict(sel_tiles=None), dict(kv_len=P + 2), dict(blocks_per_group=0),
                dict(tile=(ctypes.c_int32 * 3)(3, 3, 4))):
        assert sel(**bad) == EINVAL, bad
    assert sel(latent=(ctypes.c_int32 * 3)(64, 64, 64), tile=(ctypes.c_int32 * 3)(2, 2, 2), rows_per_tile=8) == EUNSUP
    assert sel(n_heads=0) == _C.VORTA_OK
