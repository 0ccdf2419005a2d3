"""CPU: partial geometry (tile and coreset windows that do not divide the latent grid).  The restatement of
tests/_partial_geometry_restate.py is pinned to the golden-pinned oracle on dividing geometries, then its properties and the
worked Hunyuan-129f example are checked on partial ones, and the switch is exercised at the four refusing call sites."""
import types

import numpy as np
import pytest
import torch

import _partial_geometry_restate as R
from oracle import vorta_oracle as O

DIVIDING = [((8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)), ((4, 4, 8), (2, 2, 2), (3, 5, 3), (2, 2, 2)),
            ((6, 4, 4), (6, 2, 4), (3, 3, 3), (2, 2, 2))]
PARTIAL = [((7, 5, 6), (2, 2, 4), (3, 3, 3), (2, 2, 2)), ((7, 9, 6), (2, 2, 4), (3, 3, 3), (2, 2, 2)),
           ((7, 5, 6), (8, 2, 4), (3, 3, 3), (2, 2, 2))]
HY129 = ((33, 45, 80), (6, 9, 8), (3, 3, 3), (2, 3, 2))


@pytest.fixture
def switch():
    from vorta_amd import _partial
    before = _partial._partial_geometry
    yield _partial.set_partial_geometry
    _partial._partial_geometry = before


@pytest.mark.parametrize("latent,tile,window,group", DIVIDING)
def test_restatement_equals_the_oracle_where_the_geometry_divides(latent, tile, window, group):
    assert np.array_equal(R.tile_major_order(latent, tile), O.tile_major_order(latent, tile))
    assert np.array_equal(R.sta_tile_visible(latent, tile, window), O.sta_window_tiles(latent, tile, window))
    cs, gi = R.Coreset(latent, group), O.group_info(latent, group, 0.5)
    assert np.array_equal(cs.centres, gi.center[:, 0]) and np.array_equal(cs.margins, gi.margin)
    assert cs.n_keep == gi.n_keep_margin and cs.C == 0 and cs.S_low == cs.G * (1 + cs.n_keep)
    assert len(R.key_list_lengths(latent, tile, window)) == 1


@pytest.mark.parametrize("latent,tile,window,group", PARTIAL)
def test_partial_tiles_and_windows_partition_the_grid(latent, tile, window, group):
    S = latent[0] * latent[1] * latent[2]
    order = R.tile_major_order(latent, tile)
    assert sorted(order.tolist()) == list(range(S))  # every token in exactly one tile, at one position
    tid = R.tile_id(latent, tile)[order]
    assert (np.diff(tid) >= 0).all() and tid.max() + 1 == int(np.prod(R.n_tiles(latent, tile)))
    cs = R.Coreset(latent, group)
    # every token is exactly one of centre / margin / remainder
    assert sorted(cs.centres.tolist() + cs.margins.reshape(-1).tolist() + cs.remainder.tolist()) == list(range(S))
    assert cs.C == S - cs.G * cs.g and (np.diff(cs.remainder) > 0).all()
    # the cropped windows are the reference's own (coreset_select.py:36-40, restated by the oracle)
    gi = O.group_info(latent, group, 0.5)
    assert np.array_equal(cs.centres, gi.center[:, 0]) and np.array_equal(cs.margins, gi.margin)
    # distinct key-list lengths: counted over all query tokens == derived per dimension
    seen = sorted(set(R.sta_visible(latent, tile, window).sum(1).tolist()))
    assert seen == R.key_list_lengths(latent, tile, window)


def test_key_list_length_counts_of_the_test_geometries():
    """(7,5,6): only the time axis has more tiles than the window -> two lengths.  (7,9,6): time and height each have two
    extents, (6, 5) x (6, 5) x 6 -> four combinations, of which 6*5 and 5*6 are the SAME length: three launch classes.
    (8,2,4) on (7,5,6): one thin tile spans the time axis, every window holds it -> one length."""
    n = [len(R.key_list_lengths(l, t, w)) for l, t, w, _ in PARTIAL]
    assert n == [2, 3, 1]
    assert R.key_list_lengths(*PARTIAL[1][:3]) == [150, 180, 216]
    assert R.Coreset(PARTIAL[1][0], PARTIAL[1][3]).C == 90


def test_hunyuan_129f_example():
    latent, tile, window, group = HY129
    assert R.n_tiles(latent, tile) == (6, 5, 10)
    assert [min(6, 33 - 6 * i) for i in range(6)] == [6, 6, 6, 6, 6, 3]
    fc = R.window_first_count(latent, tile, window)
    frames = [min((f + fc[0][1]) * 6, 33) - f * 6 for f in fc[0][0]]
    assert frames == [18, 18, 18, 18, 15, 15]  # query tiles t = 4, 5 see 15 frames
    assert R.key_list_lengths(latent, tile, window) == [9720, 11664]
    cs = types.SimpleNamespace(G=(33 // 2) * (45 // 3) * (80 // 2), g=12)
    cs.n_keep = int(cs.g * 0.5) - 1
    cs.C = 33 * 45 * 80 - cs.G * cs.g
    assert (cs.G, cs.n_keep, cs.C, cs.G * (1 + cs.n_keep) + cs.C) == (9600, 5, 3600, 61200)
    # the host geometry and the library's size query agree
    from vorta_amd import ops
    from vorta_amd.routed import RoutedGeometry
    g = RoutedGeometry(latent, tile, window, group, 0.5, torch.device("cpu"), partial=True)
    assert (g.G, g.n_keep, g.C, g.S_low, g.is_partial) == (9600, 5, 3600, 61200, True)
    assert g.sta_class_n_kv == [11664, 9720]
    n_tiles, n_lists, stride, lens = ops.sta_partial_sizes(latent, tile, window, 96)
    assert (n_tiles, n_lists, stride) == (300, 4 * 3 * 8, 11664 + 96) and sorted(set(lens)) == [9720 + 96, 11664 + 96]


@pytest.mark.parametrize("latent,tile,window,group", PARTIAL)
def test_host_geometry_matches_the_restatement(latent, tile, window, group):
    from vorta_amd import ops
    from vorta_amd.routed import RoutedGeometry
    g = RoutedGeometry(latent, tile, window, group, 0.5, torch.device("cpu"), partial=True)
    cs = R.Coreset(latent, group)
    assert (g.G, g.C, g.S_low, g.n_keep) == (cs.G, cs.C, cs.S_low, cs.n_keep)
    assert sorted(g.sta_class_n_kv) == R.key_list_lengths(latent, tile, window)
    assert sorted(set(ops.sta_partial_sizes(latent, tile, window, 0)[3])) == R.key_list_lengths(latent, tile, window)


def test_dividing_geometry_is_the_same_object_either_way():
    from vorta_amd.routed import RoutedGeometry
    a = RoutedGeometry(*DIVIDING[0], 0.5, torch.device("cpu"), partial=False)
    b = RoutedGeometry(*DIVIDING[0], 0.5, torch.device("cpu"), partial=True)
    assert not b.is_partial and (a.G, a.C, a.S_low, a.tok, a.sta_class_n_kv) == (b.G, b.C, b.S_low, b.tok, b.sta_class_n_kv)


def _refusing_sites(latent, tile, window, group):
    """the four host call sites that refuse a non-dividing geometry, as callables"""
    from vorta_amd.attention import create_sliding_tile_attn_mask_func, get_group_info
    from vorta_amd.attention.hunyuan import HunyuanVideoFlashAttnProcessorTripleEval
    from vorta_amd.attention.wan import WanAttnProcessorTripleEval
    from vorta_amd.patch.utils import validate_geometry
    from vorta_amd.routed import RoutedGeometry
    S = latent[0] * latent[1] * latent[2]
    hs = torch.zeros((1, S, 8))
    gi = get_group_info(latent, group, 0.5)
    kw = dict(latent_shape=latent, tile_size=tile, window_size=window, lowres_window_size=group, lowres_reduction_rate=0.5)
    return {
        "RoutedGeometry": lambda: RoutedGeometry(latent, tile, window, group, 0.5, torch.device("cpu")),
        "validate_geometry": lambda: validate_geometry(dict(kw)),
        "create_sliding_tile_attn_mask_func": lambda: create_sliding_tile_attn_mask_func(latent, window, tile, 0, 0, "cpu"),
        "hunyuan._check_input": lambda: HunyuanVideoFlashAttnProcessorTripleEval(check_input=True)._check_input(
            hs, gi, latent, window, tile),
        "wan._check_input": lambda: WanAttnProcessorTripleEval(check_input=True)._check_input(hs, gi, latent, window, tile),
    }


def test_switch_off_keeps_todays_refusals_and_on_lifts_them(switch):
    latent, tile, window, group = PARTIAL[1]
    switch(False)
    for name, fn in _refusing_sites(latent, tile, window, group).items():
        with pytest.raises(ValueError, match=r"Tile size \(2, 2, 4\) \(dim=2\) does not divide latent shape \(7, 9, 6\) \(dim=7\)\."):
            fn()
    # a tile that divides and a coreset window that does not: the second message of each site
    sites = _refusing_sites((6, 4, 4), (2, 2, 2), window, (4, 2, 2))
    with pytest.raises(ValueError, match=r"Input sequence length 96 does not match low-res info 4x16\."):
        sites["RoutedGeometry"]()
    with pytest.raises(ValueError, match=r"Low-res window \(4, 2, 2\) \(dim=4\) does not divide latent shape \(6, 4, 4\)"):
        sites["validate_geometry"]()
    for name in ("hunyuan._check_input", "wan._check_input"):
        with pytest.raises(ValueError, match=r"Input sequence length 96 does not match low-res info 4x16\."):
            sites[name]()
    switch(True)
    for lat, til, grp in ((latent, tile, group), ((6, 4, 4), (2, 2, 2), (4, 2, 2))):
        for name, fn in _refusing_sites(lat, til, window, grp).items():
            fn()
    g = _refusing_sites(latent, tile, window, group)["RoutedGeometry"]()
    assert g.is_partial and g.C == 90
    # a coreset window larger than the grid has no whole window: refused either way
    with pytest.raises(ValueError, match="no whole window"):
        _refusing_sites((7, 5, 6), (2, 2, 4), window, (8, 2, 2))["RoutedGeometry"]()
    with pytest.raises(ValueError, match="no whole window"):
        _refusing_sites((7, 5, 6), (2, 2, 4), window, (8, 2, 2))["validate_geometry"]()


def test_switch_reads_the_environment_and_keys_the_cache(switch, monkeypatch):
    import vorta_amd
    from vorta_amd import _partial
    from vorta_amd.routed import geometry_for
    _partial._partial_geometry = None
    monkeypatch.delenv("VORTA_PARTIAL_GEOMETRY", raising=False)
    assert _partial.partial_geometry() is False  # the default is off
    monkeypatch.setenv("VORTA_PARTIAL_GEOMETRY", "1")
    assert _partial.partial_geometry() is True
    vorta_amd.set_partial_geometry(False)  # the call overrides the environment
    assert _partial.partial_geometry() is False
    a = geometry_for(*DIVIDING[0], 0.5, "cpu")
    b = geometry_for(*DIVIDING[0], 0.5, "cpu", partial=True)
    assert a is not b and a is geometry_for(*DIVIDING[0], 0.5, "cpu", partial=False)
    vorta_amd.set_partial_geometry(True)
    assert geometry_for(*DIVIDING[0], 0.5, "cpu") is b
    assert geometry_for(*PARTIAL[0], 0.5, "cpu").is_partial


def test_library_keeps_refusing_through_the_old_entry_points():
    """vorta_sta_table_sizes still returns VORTA_EINVAL for a tile that does not divide (-> ValueError)"""
    from vorta_amd import ops
    with pytest.raises(ValueError, match="vorta_sta_table_sizes"):
        ops.sta_table_sizes(PARTIAL[0][0], PARTIAL[0][1], PARTIAL[0][2], 0)


@pytest.mark.parametrize("latent,tile,window,group", PARTIAL + DIVIDING + [((7, 7, 7), (2, 2, 2), (3, 3, 3), (2, 2, 2))])
def test_host_work_formulas_count_the_restatements_pairs(latent, tile, window, group, switch):
    """the (query, key) pair count behind the sequence-parallel placement cost and `patch.fidelity.expert_work`, and S_low"""
    from vorta_amd import _partial
    switch(True)
    from vorta_amd.patch.fidelity import expert_work
    S = latent[0] * latent[1] * latent[2]
    pairs = int(R.sta_visible(latent, tile, window).sum())
    assert _partial.sliding_video_pairs(latent, tile, window) == pairs
    cs = R.Coreset(latent, group)
    assert _partial.coreset_numbers(latent, group, 0.5) == (cs.G, cs.n_keep, cs.C, cs.S_low)
    te, D = 7, 128
    geometry = dict(latent=latent, tile=tile, window=window, group=group, rate=0.5)
    want = (4.0 * (S + te) ** 2 * D, 4.0 * (cs.S_low + te) ** 2 * D, 4.0 * D * (pairs + S * te + te * (S + te)))
    assert expert_work(geometry, te) == pytest.approx(want, rel=1e-12)
    from vorta_amd.routed import RoutedGeometry
    assert expert_work(RoutedGeometry(device=torch.device("cpu"), **geometry), te) == expert_work(geometry, te)


def test_expert_work_of_the_129f_example(switch):
    from vorta_amd.patch.fidelity import _geometry_numbers
    switch(True)
    latent, tile, window, group = HY129
    S, s_low, _, keys = _geometry_numbers(dict(latent=latent, tile=tile, window=window, group=group, rate=0.5))
    assert (S, s_low) == (118800, 61200)
    assert keys == pytest.approx((24 * 11664 + 9 * 9720) / 33)  # 24 frames of query tiles see 18 frames, 9 see 15


def test_check_input_still_catches_a_group_info_of_another_latent(switch):
    from vorta_amd.attention import get_group_info
    from vorta_amd.attention.wan import WanAttnProcessorTripleEval
    proc = WanAttnProcessorTripleEval(check_input=True)
    switch(True)
    # a geometry that divides is checked as with the switch off
    latent, tile, window, group = DIVIDING[0]
    hs = torch.zeros((1, latent[0] * latent[1] * latent[2], 8))
    proc._check_input(hs, get_group_info(latent, group, 0.5), latent, window, tile)
    with pytest.raises(ValueError, match=r"Input sequence length 384 does not match low-res info 16x12\."):
        proc._check_input(hs, get_group_info((4, 6, 8), group, 0.5), latent, window, tile)
    # a partial one: the group info must be the cropped windows of this latent shape
    latent, tile, window, group = PARTIAL[1]
    hs = torch.zeros((1, latent[0] * latent[1] * latent[2], 8))
    proc._check_input(hs, get_group_info(latent, group, 0.5), latent, window, tile)
    with pytest.raises(ValueError, match="was not built for latent shape"):
        proc._check_input(hs, get_group_info((7, 5, 6), group, 0.5), latent, window, tile)
