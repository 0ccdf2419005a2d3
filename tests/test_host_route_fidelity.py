"""Host side of routing by measured statistics (no GPU): `routes_from_fidelity(max_flops_share=...)` -- the FLOP-budget rule
that `ops.route_fidelity` (vorta_route_fidelity) applies on the device and that this function DEFINES -- on hand-made records;
today's positional calls, pinned; the refusals; the library's argument checks, which return before anything is launched."""
import ctypes
import math

import pytest
import torch

GEOMETRY = dict(latent=(33, 45, 80), tile=(11, 9, 8), window=(3, 3, 3), group=(2, 3, 2), rate=0.5)
NAN, INF = float("nan"), float("inf")


def _fid(sq_ref, sq_err):
    from vorta_amd.ops import ExpertFidelity
    sq_ref, sq_err = torch.tensor(sq_ref, dtype=torch.float32), torch.tensor(sq_err, dtype=torch.float32)
    return ExpertFidelity(sq_ref, sq_ref.sqrt(), sq_err, sq_err.sqrt(), None, 128)


def _budget(sq_ref, sq_err, share, work):
    from vorta_amd.patch import routes_from_fidelity
    return routes_from_fidelity(_fid(sq_ref, sq_err), geometry=dict(work=work), max_flops_share=share).tolist()


# four heads whose sliding tile (column 1) is 0.1 off and whose coreset is far off; work 4 / 2 / 1: every move saves 3 of 16
EQUAL = [[4.0, 0.01, 9.0]] * 4


def test_equal_errors_move_the_lower_head_first():
    assert _budget([1.0] * 4, EQUAL, 0.8, (4.0, 2.0, 1.0)) == [2, 2, 0, 0]   # 16 > 12.8, 13 > 12.8, 10 <= 12.8
    assert _budget([1.0] * 4, EQUAL, 0.9, (4.0, 2.0, 1.0)) == [2, 0, 0, 0]


def test_smaller_errors_move_first_whatever_the_head():
    err = [[4.0, 0.04, 9.0], [0.01, 4.0, 9.0], [4.0, 0.0004, 9.0], [4.0, 0.09, 9.0]]
    # ranking by rel: head 2 (0.02, sliding), head 1 (0.1, coreset), head 0 (0.2), head 3 (0.3)
    assert _budget([1.0] * 4, err, 0.99, (4.0, 2.0, 1.0)) == [0, 0, 2, 0]
    assert _budget([1.0] * 4, err, 0.80, (4.0, 2.0, 1.0)) == [0, 1, 2, 0]   # 16, 13 > 12.8; 11 <= 12.8
    assert _budget([1.0] * 4, err, 0.60, (4.0, 2.0, 1.0)) == [2, 1, 2, 0]   # 11 > 9.6; 8 <= 9.6


def test_a_budget_met_exactly_stops_the_walk():
    # 0.625 * 16 = 10 exactly: after two moves the cost IS the budget, and `cost > budget` no longer holds
    assert _budget([1.0] * 4, EQUAL, 0.625, (4.0, 2.0, 1.0)) == [2, 2, 0, 0]
    assert _budget([1.0] * 4, EQUAL, math.nextafter(0.625, 0.0), (4.0, 2.0, 1.0)) == [2, 2, 2, 0]


def test_an_unreachable_budget_moves_every_candidate_and_nothing_else():
    err = [[4.0, 0.01, 9.0], [NAN, NAN, 9.0], [0.04, 4.0, 9.0], [INF, NAN, 9.0]]
    assert _budget([1.0] * 4, err, 0.01, (4.0, 2.0, 1.0)) == [2, 0, 1, 0]
    # sq_ref == 0: rel is 0 where the error is 0 (a candidate) and inf otherwise (never one)
    assert _budget([0.0, 0.0, 1.0], [[0.0, 1.0, 9.0], [1.0, 2.0, 9.0], [NAN, 0.25, 9.0]], 0.01, (4.0, 2.0, 1.0)) == [1, 0, 2]


def test_a_share_of_one_or_more_moves_nothing():
    for share in (1.0, 1.5, INF):
        assert _budget([1.0] * 4, EQUAL, share, (4.0, 2.0, 1.0)) == [0, 0, 0, 0]


def test_a_nan_or_inf_candidate_is_never_moved():
    err = [[NAN, INF, 9.0], [INF, 0.01, 9.0], [0.01, NAN, 9.0]]
    assert _budget([1.0] * 3, err, 0.01, (4.0, 2.0, 1.0)) == [0, 2, 1]


def test_an_expert_that_costs_what_full_attention_costs_is_no_candidate():
    err = [[0.0, 0.01, 9.0], [0.0, NAN, 9.0]]
    assert _budget([1.0] * 2, err, 0.01, (4.0, 4.0, 1.0)) == [2, 0]      # coreset is exact and still never taken
    assert _budget([1.0] * 2, err, 0.01, (4.0, 5.0, 4.0)) == [0, 0]
    assert _budget([1.0] * 2, err, 0.01, (4.0, 1.0, 6.0)) == [1, 1]


def test_the_candidate_of_a_head_on_equal_errors():
    err = [[0.01, 0.01, 9.0]]
    assert _budget([1.0], err, 0.01, (4.0, 1.0, 2.0)) == [1]   # the smaller work
    assert _budget([1.0], err, 0.01, (4.0, 2.0, 1.0)) == [2]
    assert _budget([1.0], err, 0.01, (4.0, 2.0, 2.0)) == [2]   # equal work: expert 2
    assert _budget([1.0], [[0.01, 0.04, 9.0]], 0.01, (4.0, 3.0, 1.0)) == [1]  # the smaller error wins over the smaller work


def test_leading_dimensions():
    from vorta_amd.patch import routes_from_fidelity
    g = torch.Generator().manual_seed(3)
    choices = torch.tensor([0.0, 0.0004, 0.01, 0.01, 0.09, 4.0, NAN, INF])
    sq_err = choices[torch.randint(0, len(choices), (2, 3, 5, 3), generator=g)]
    sq_ref = torch.tensor([0.0, 1.0, 1.0, 1.0])[torch.randint(0, 4, (2, 3, 5), generator=g)]
    geometry = dict(work=(5.0, 2.0, 1.5))
    fid = _fid(sq_ref.tolist(), sq_err.tolist())
    table = routes_from_fidelity(fid, geometry=geometry, max_flops_share=0.6)
    assert table.shape == (2, 3, 5) and table.dtype == torch.int64
    seen = set()
    for a in range(2):
        for b in range(3):
            one = routes_from_fidelity(_fid(sq_ref[a, b].tolist(), sq_err[a, b].tolist()), geometry=geometry, max_flops_share=0.6)
            assert one.tolist() == table[a, b].tolist()
            seen |= set(one.tolist())
    assert len(seen) > 1
    # a real geometry: its work comes from the formulas (sliding tile cheapest at this one)
    assert routes_from_fidelity(_fid([1.0] * 4, EQUAL), geometry=GEOMETRY, max_flops_share=1e-3).tolist() == [2, 2, 2, 2]


def test_positional_calls_return_what_they_returned():
    from vorta_amd.patch import routes_from_fidelity
    f = _fid([[1.0] * 7], [[[0.0004, 0.0009, 9.0], [0.0004, 0.25, 9.0], [0.25, 0.0004, 9.0], [0.25, 0.25, 9.0],
                            [0.0025, 0.0025, 9.0], [0.0, 0.04, 9.0], [NAN, NAN, 9.0]]])
    assert routes_from_fidelity(f, 0.05).tolist() == [[2, 1, 2, 0, 2, 1, 0]]
    assert routes_from_fidelity(f, 0.05, GEOMETRY).tolist() == [[2, 1, 2, 0, 2, 1, 0]]
    assert routes_from_fidelity(f, 0.05, dict(GEOMETRY, window=(3, 5, 10)), 0).tolist() == [[1, 1, 2, 0, 1, 1, 0]]
    assert routes_from_fidelity(f, 0.0).tolist() == [[0, 0, 0, 0, 0, 1, 0]]


def test_refusals():
    from vorta_amd.patch import routes_from_fidelity
    f = _fid([1.0] * 4, EQUAL)
    with pytest.raises(ValueError, match="exactly one of max_rel_error and max_flops_share"):
        routes_from_fidelity(f)
    with pytest.raises(ValueError, match="exactly one of max_rel_error and max_flops_share"):
        routes_from_fidelity(f, 0.05, GEOMETRY, max_flops_share=0.5)
    with pytest.raises(ValueError, match="max_flops_share needs `geometry`"):
        routes_from_fidelity(f, max_flops_share=0.5)
    with pytest.raises(ValueError, match="max_flops_share"):
        routes_from_fidelity(f, geometry=GEOMETRY, max_flops_share=0.0)


def test_surface_and_argument_checks_before_any_launch():
    """the new names are exported; vorta_route_fidelity returns VORTA_EINVAL on the host for every bad argument"""
    import vorta_amd.torch_ops  # noqa: F401
    from vorta_amd import _C, ops, patch, routed
    for name in ("measured_routes", "measured_routes_of"):
        assert callable(getattr(patch, name))
    assert callable(ops.route_fidelity) and callable(routed.route_by_fidelity)
    assert "route_fidelity" in dir(torch.ops.vorta)
    schema = str(torch.ops.vorta.route_fidelity.default._schema)
    assert "float? max_rel_error=None" in schema and "float[]? work=None" in schema and schema.endswith("(Tensor, Tensor, Tensor, Tensor)")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():  # the shape function, usable without a GPU
        e, lists, counts, share = torch.ops.vorta.route_fidelity(torch.empty((6,), device="cuda"), torch.empty((6, 3), device="cuda"),
                                                                 max_flops_share=0.5, work=[3.0, 2.0, 1.0])
        assert e.shape == (6,) and lists.shape == (3, 6) and counts.shape == (3,) and share.shape == (1,)
        assert e.dtype == lists.dtype == counts.dtype == torch.int32 and share.dtype == torch.float32
    lib = _C.lib()
    assert lib.vorta_route_fidelity_args_size() == ctypes.sizeof(_C.RouteFidelityArgs)
    buf = (ctypes.c_float * 16)()
    where = ctypes.addressof(buf)

    def args(**kw):
        a = _C.RouteFidelityArgs()
        a.struct_size, a.heads, a.mode, a.max_rel_error, a.max_flops_share = ctypes.sizeof(a), 4, 0, 0.05, 0.5
        a.sq_ref = a.sq_err = a.expert_of_head = a.head_lists = a.head_counts = where
        for e, w in enumerate(kw.pop("work", (3.0, 2.0, 1.0))):
            a.work[e] = w
        for key, value in kw.items():
            setattr(a, key, value)
        return a

    bad = [dict(struct_size=8), dict(heads=0), dict(heads=1025), dict(mode=2), dict(mode=-1), dict(sq_ref=None),
           dict(sq_err=None), dict(expert_of_head=None), dict(head_lists=None), dict(head_counts=None),
           dict(max_rel_error=-0.5), dict(max_rel_error=NAN), dict(mode=1, max_flops_share=0.0),
           dict(mode=1, max_flops_share=-1.0), dict(mode=1, max_flops_share=NAN), dict(work=(0.0, 2.0, 1.0)),
           dict(work=(3.0, -2.0, 1.0)), dict(work=(3.0, 2.0, INF)), dict(work=(3.0, NAN, 1.0))]
    for kw in bad:
        assert lib.vorta_route_fidelity(ctypes.byref(args(**kw)), None) == _C.VORTA_EINVAL, kw
    assert lib.vorta_route_fidelity(None, None) == _C.VORTA_EINVAL
    with pytest.raises(ValueError, match="exactly one"):
        ops.route_fidelity(_fid([1.0] * 4, EQUAL))
    with pytest.raises(ValueError, match="exactly one"):
        routed.route_by_fidelity(None, None, None, None, model="wan", max_rel_error=0.1, max_flops_share=0.5)
    rule = routed.RouteRule("max_rel_error", 0.05)
    assert (rule.n_rows, rule.seed) == (512, 0)
    with pytest.raises(ValueError, match="RouteRule"):
        routed.RouteRule("tau", 0.05)
    with pytest.raises(Exception):  # frozen
        rule.value = 0.1
