"""Host: the `sliding_keys` switch -- keyword, then `set_sliding_keys`, then VORTA_SLIDING_KEYS, then "window" --, unknown names,
and the refusals a "content" geometry makes when it is built (no GPU: a geometry builds its tables on first use)."""
import pytest
import torch

GEOMETRY = ((8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2), 0.5, torch.device("cpu"))


def test_precedence_keyword_then_setter_then_environment(monkeypatch):
    import vorta_amd
    from vorta_amd import routed
    monkeypatch.setattr(routed, "_sliding_keys", None)
    monkeypatch.delenv("VORTA_SLIDING_KEYS", raising=False)
    assert routed.sliding_keys_of() == "window" and routed.RoutedGeometry(*GEOMETRY).sliding_keys == "window"
    monkeypatch.setenv("VORTA_SLIDING_KEYS", "content")
    assert routed.RoutedGeometry(*GEOMETRY).sliding_keys == "content"
    vorta_amd.set_sliding_keys("window")  # the setter overrides the environment
    assert routed.RoutedGeometry(*GEOMETRY).sliding_keys == "window"
    assert routed.RoutedGeometry(*GEOMETRY, sliding_keys="content").sliding_keys == "content"  # the keyword overrides both
    a, b = (routed.geometry_for(*GEOMETRY, sliding_keys=name) for name in ("window", "content"))
    assert a is not b and a is routed.geometry_for(*GEOMETRY) and b.sliding_keys == "content"


@pytest.mark.parametrize("how", ["keyword", "setter", "environment"])
def test_unknown_names_are_errors(how, monkeypatch):
    from vorta_amd import routed
    monkeypatch.setattr(routed, "_sliding_keys", None)
    with pytest.raises(ValueError, match="unknown sliding keys 'nearest'.*window, content"):
        if how == "keyword":
            routed.RoutedGeometry(*GEOMETRY, sliding_keys="nearest")
        elif how == "setter":
            routed.set_sliding_keys("nearest")
        else:
            monkeypatch.setenv("VORTA_SLIDING_KEYS", "nearest")
            routed.RoutedGeometry(*GEOMETRY)


def test_content_refuses_partial_geometry_and_sequence_parallelism():
    from vorta_amd.routed import RoutedGeometry
    with pytest.raises(ValueError, match="partial geometry.*tiles of different thickness are missing"):
        RoutedGeometry((9, 6, 8), *GEOMETRY[1:], partial=True, sliding_keys="content")
    with pytest.raises(ValueError, match="sequence parallelism.*not wired into the sequence-parallel engine"):
        RoutedGeometry(*GEOMETRY, row_map=torch.arange(8 * 6 * 8, dtype=torch.int32), sliding_keys="content")
    assert RoutedGeometry(*GEOMETRY, partial=True, sliding_keys="content").is_partial is False  # (a geometry that divides)
