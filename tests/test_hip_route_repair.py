"""GPU: `ops.route_repair` (vorta_route_repair) against the host rule, `vorta.patch.repair_routes`, which is the definition.
The route tables after the call (updated in place), the repair list up to its count, the count, the state and rel must be
EQUAL -- no tolerance: rel is two correctly rounded float32 operations.

The crafted records of tests/test_host_route_repair.py; seeded random records with errors from a small set, so that heads on
and over the bound are common, at H in {1, 5, 24, 40, 1024} x 1..3 tiers with the exact tier at every index; the sentinel past
a count; the error codes, which leave every buffer untouched; the operator; a captured graph whose replays follow the
record in the buffers and read the tables the replay before left."""
import ctypes as C

import pytest
import torch

from _util import dev
from test_host_route_repair import EXPERTS, SQ_ERR, SQ_REF

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
REFS = [0.0, 1.0, 4.0, 16.0, 16.0, 16.0, NAN]
ERRS = [0.0, 0.25, 1.0, 1.0, 4.0, 9.0, 9.0, 16.0, 3.0, 1e-30, NAN, INF]
BOUNDS = [0.0, 0.25, 0.5, 0.75, 1.0, 0.4330127, 3.0, INF]
SENTINEL = -7


def _record(H, n_tiers, seed):
    """(experts, tiers, exact, sq_ref, sq_err, bound) of one drawn case: experts in -1..2, tiers in 0..n_tiers-1"""
    g = torch.Generator().manual_seed(100000 * n_tiers + 1000 * H + seed)
    pick = lambda values, shape: torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]  # noqa: E731
    experts = torch.randint(-1, 3, (H,), generator=g).to(torch.int32)
    tiers = torch.randint(0, n_tiers, (H,), generator=g).to(torch.int32)
    exact = int(torch.randint(0, n_tiers, (1,), generator=g))
    return experts, tiers, exact, pick(REFS, (H,)), pick(ERRS, (H,)), BOUNDS[int(torch.randint(0, len(BOUNDS), (1,), generator=g))]


def _device_tables(experts, tiers, n_tiers):
    """the device tables of a case before the call: lists and counts hold the SENTINEL (the kernel rebuilds them from the head
    tables and does not read them)"""
    H = experts.numel()
    return (experts.clone().to(dev()), None if tiers is None else tiers.clone().to(dev()),
            torch.full((n_tiers, 3, H), SENTINEL, dtype=torch.int32, device=dev()),
            torch.full((n_tiers, 3), SENTINEL, dtype=torch.int32, device=dev()))


def _outs(H):
    return (torch.full((H,), SENTINEL, dtype=torch.int32, device=dev()), torch.full((1,), SENTINEL, dtype=torch.int32, device=dev()),
            torch.full((H,), SENTINEL, dtype=torch.int32, device=dev()), torch.full((H,), -7.0, dtype=torch.float32, device=dev()))


def _same_floats(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0, 1e30, -1e30), b.nan_to_num(0.0, 1e30, -1e30))


def _check(tables, outs, want, case):
    """the device tables and outputs of one call (already on the host) against the host rule's"""
    expert, tier, lists, counts = tables
    repair_list, repair_count, state, rel = outs
    H = expert.numel()
    assert expert.tolist() == want.expert_of_head.tolist(), f"{case}: expert table"
    if tier is not None:
        assert tier.tolist() == want.tier_of_head.tolist(), f"{case}: tier table"
    assert counts.tolist() == want.counts.tolist(), f"{case}: counts"
    for t in range(counts.shape[0]):
        for e in range(3):
            n = int(want.counts[t, e])
            # up to the count the host's list; past it the sentinel: not written
            assert lists[t, e].tolist() == want.lists[t, e, :n].tolist() + [SENTINEL] * (H - n), f"{case}: list ({t}, {e})"
    n = want.repair_count
    assert int(repair_count) == n and repair_list.tolist() == want.repair_list[:n].tolist() + [SENTINEL] * (H - n), f"{case}: repairs"
    assert state.tolist() == want.state_of_head.tolist(), f"{case}: state"
    assert _same_floats(rel, want.rel), f"{case}: rel {rel.tolist()} != host {want.rel.tolist()}"


def _run(sq_ref, sq_err, tables, exact, bound, outs=None):
    from vorta_amd import ops
    return ops.route_repair(sq_ref.to(dev()), sq_err.to(dev()), *tables, exact_tier=exact, repair_above=bound, out=outs)


def _host(experts, tiers, n_tiers, exact, sq_ref, sq_err, bound):
    from vorta_amd.patch import repair_routes
    return repair_routes(experts, tiers, n_tiers, exact, sq_ref, sq_err, bound)


def _cpu(ts):
    return [None if t is None else t.cpu() for t in ts]


def test_crafted_records_equal_the_host_rule_bit_for_bit():
    experts = torch.tensor(EXPERTS, dtype=torch.int32)
    ref, err = torch.tensor(SQ_REF), torch.tensor(SQ_ERR)
    H = experts.numel()
    for n_tiers in (1, 2, 3):
        for exact in range(n_tiers):
            for shift in range(n_tiers):
                tiers = torch.tensor([(h + shift) % n_tiers for h in range(H)], dtype=torch.int32)
                for with_tiers in ((False, True) if n_tiers == 1 else (True,)):  # (NULL tier_of_head goes with one tier)
                    for bound in (0.0, 0.75, 0.7499999, 0.75 + 1e-9, INF):
                        tables = _device_tables(experts, tiers if with_tiers else None, n_tiers)
                        outs = _run(ref, err, tables, exact, bound, _outs(H))
                        assert all(t.is_cuda for t in outs)
                        _check(_cpu(tables), _cpu(outs), _host(experts, tiers, n_tiers, exact, ref, err, bound),
                               f"crafted n_tiers={n_tiers} exact={exact} shift={shift} bound={bound}")


@pytest.mark.parametrize("n_tiers", [1, 2, 3])
@pytest.mark.parametrize("H", [1, 5, 24, 40, 1024])
def test_random_records_equal_the_host_rule(H, n_tiers):
    seeds = 8 if H == 1024 else 60
    cases, got = [], []
    for seed in range(seeds):
        case = _record(H, n_tiers, seed)
        experts, tiers, exact, sq_ref, sq_err, bound = case
        tables = _device_tables(experts, tiers, n_tiers)
        cases.append(case)
        got.append((tables, _run(sq_ref, sq_err, tables, exact, bound, _outs(H))))
    torch.cuda.synchronize()
    seen = set()
    for seed, (case, (tables, outs)) in enumerate(zip(cases, got)):
        experts, tiers, exact, sq_ref, sq_err, bound = case
        want = _host(experts, tiers, n_tiers, exact, sq_ref, sq_err, bound)
        _check(_cpu(tables), _cpu(outs), want, f"H={H} n_tiers={n_tiers} seed={seed} exact={exact} bound={bound}")
        seen.add(tuple(want.state_of_head.tolist()))
        # idempotent on the device too: the same record on the repaired tables repairs nothing and leaves them as they are
        before = [t.clone() for t in tables]
        again = _run(sq_ref, sq_err, tables, exact, bound)
        assert int(again[1]) == 0 and not bool((again[2] == 2).any()), (H, seed)
        assert torch.equal(tables[0], before[0]) and torch.equal(tables[1], before[1]) and torch.equal(tables[3], before[3])
    assert len(seen) >= (2 if H == 1 else 6)  # the draws do exercise the rule


def test_arbitrary_floats_round_as_the_host_does():
    """records whose rel is no short binary fraction: the divide and the square root must round as the host's do, to the bit,
    and a bound that IS one head's rel keeps that head on the device too"""
    H = 1024
    g = torch.Generator().manual_seed(5)
    experts, tiers = torch.ones(H, dtype=torch.int32), torch.zeros(H, dtype=torch.int32)
    for scale in (1.0, 1e-3, 3e3):
        sq_ref = (torch.rand(H, generator=g) * 3000 + 1e-3).float()
        sq_err = (torch.rand(H, generator=g) * sq_ref * scale).float()
        probe = _host(experts, tiers, 1, 0, sq_ref, sq_err, 1.0)
        for bound in (1.0, float(probe.rel[17]), float(probe.rel.median())):
            tables = _device_tables(experts, tiers, 1)
            outs = _run(sq_ref, sq_err, tables, 0, bound, _outs(H))
            want = _host(experts, tiers, 1, 0, sq_ref, sq_err, bound)
            _check(_cpu(tables), _cpu(outs), want, f"arbitrary floats scale={scale} bound={bound}")
        assert want.state_of_head[int(probe.rel.argsort()[H // 2 - 1])] == 1  # (the lower median: on the bound, kept)


def _raw_args(ref_t, err_t, tables, outs, **kw):
    from vorta_amd import _C
    a = _C.RouteRepairArgs()
    a.struct_size, a.heads, a.n_tiers, a.exact_tier, a.repair_above = C.sizeof(a), ref_t.numel(), 2, 1, 0.75
    a.sq_ref, a.sq_err = ref_t.data_ptr(), err_t.data_ptr()
    a.expert_of_head, a.tier_of_head, a.head_lists, a.head_counts = (t.data_ptr() for t in tables)
    a.repair_list, a.repair_count, a.state_of_head, a.rel = (t.data_ptr() for t in outs)
    for key, value in kw.items():
        setattr(a, key, value)
    return a


def test_error_codes_leave_every_buffer_untouched():
    from vorta_amd import _C, ops
    experts = torch.tensor(EXPERTS, dtype=torch.int32)
    H = experts.numel()
    tiers = torch.tensor([h % 2 for h in range(H)], dtype=torch.int32)
    sq_ref, sq_err = torch.tensor(SQ_REF, device=dev()), torch.tensor(SQ_ERR, device=dev())
    tables, outs = _device_tables(experts, tiers, 2), _outs(H)
    before = [t.clone() for t in tables + outs]
    lib, stream = _C.lib(), torch.cuda.current_stream().cuda_stream
    bad = [dict(heads=1025), dict(heads=0), dict(n_tiers=0), dict(n_tiers=4), dict(exact_tier=-1), dict(exact_tier=2),
           dict(sq_ref=None), dict(sq_err=None), dict(expert_of_head=None), dict(tier_of_head=None), dict(head_lists=None),
           dict(head_counts=None), dict(repair_list=None), dict(repair_count=None), dict(repair_above=-0.5),
           dict(repair_above=NAN), dict(struct_size=C.sizeof(_C.RouteRepairArgs) - 8)]
    for kw in bad:
        assert lib.vorta_route_repair(C.byref(_raw_args(sq_ref, sq_err, tables, outs, **kw)), stream) == _C.VORTA_EINVAL, kw
    assert lib.vorta_route_repair(None, stream) == _C.VORTA_EINVAL
    torch.cuda.synchronize()
    for t, b in zip(tables + outs, before):
        assert torch.equal(t, b) or _same_floats(t, b), "a refused call wrote a buffer"
    # the same block, accepted; and without the optional outputs
    assert lib.vorta_route_repair(C.byref(_raw_args(sq_ref, sq_err, tables, outs)), stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    want = _host(experts, tiers, 2, 1, SQ_REF, SQ_ERR, 0.75)
    _check(_cpu(tables), _cpu(outs), want, "raw call")
    assert int(want.counts.sum()) < 6 * H and want.repair_count < H  # (some sentinel does survive)
    tables2, outs2 = _device_tables(experts, tiers, 2), _outs(H)
    assert lib.vorta_route_repair(C.byref(_raw_args(sq_ref, sq_err, tables2, outs2, state_of_head=None, rel=None)),
                                  stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(tables2, tables)) and torch.equal(outs2[0], outs[0])
    assert bool((outs2[2] == SENTINEL).all()) and bool((outs2[3] == -7.0).all())
    # the launcher's own refusals
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev())  # noqa: E731
    with pytest.raises(ValueError, match="vorta_route_repair"):
        ops.route_repair(sq_ref, sq_err, i32(H), i32(H), i32(2, 3, H), i32(2, 3), exact_tier=2, repair_above=0.5)
    with pytest.raises(ValueError, match="vorta_route_repair"):
        ops.route_repair(sq_ref, sq_err, i32(H), i32(H), i32(2, 3, H), i32(2, 3), exact_tier=0, repair_above=-1.0)
    with pytest.raises(ValueError, match="vorta_route_repair"):
        ops.route_repair(sq_ref, sq_err, i32(H), None, i32(2, 3, H), i32(2, 3), exact_tier=0, repair_above=0.5)
    with pytest.raises(ValueError, match="ONE layer"):
        ops.route_repair(sq_ref[None], sq_err[None], i32(H), None, i32(3, H), i32(3), exact_tier=0, repair_above=0.5)
    with pytest.raises(ValueError, match="in place"):
        ops.route_repair(sq_ref, sq_err, i32(H).long(), None, i32(3, H), i32(3), exact_tier=0, repair_above=0.5)
    with pytest.raises(ValueError, match="head_lists"):
        ops.route_repair(sq_ref, sq_err, i32(H), None, i32(3, H + 1), i32(3), exact_tier=0, repair_above=0.5)


def test_one_tier_takes_the_tables_of_a_head_routing():
    """(3, H) lists and (3,) counts, no tier table: the form `HeadRouting.from_device` holds"""
    from vorta_amd import ops
    experts = torch.tensor(EXPERTS, dtype=torch.int32)
    H = experts.numel()
    ids = experts.clone().to(dev())
    lists = torch.full((3, H), SENTINEL, dtype=torch.int32, device=dev())
    counts = torch.full((3,), SENTINEL, dtype=torch.int32, device=dev())
    outs = ops.route_repair(torch.tensor(SQ_REF, device=dev()), torch.tensor(SQ_ERR, device=dev()), ids, None, lists, counts,
                            exact_tier=0, repair_above=0.75, out=_outs(H))
    _check(_cpu((ids, None, lists.view(1, 3, H), counts.view(1, 3))), _cpu(outs),
           _host(experts, None, 1, 0, SQ_REF, SQ_ERR, 0.75), "head routing tables")


def test_graph_replays_follow_the_record_and_read_the_tables_the_replay_before_left():
    H, n_tiers = 40, 3
    experts, tiers, exact, sq_ref, sq_err, _ = _record(H, n_tiers, 0)
    bound = 0.5
    ref_d, err_d = sq_ref.to(dev()), sq_err.to(dev())
    tables = _device_tables(experts, tiers, n_tiers)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks, on tables of its own
        _run(ref_d, err_d, _device_tables(experts, tiers, n_tiers), exact, bound)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _run(ref_d, err_d, tables, exact, bound)
    tables[0].copy_(experts)  # (capture launches nothing; the tables start from the case's)
    tables[1].copy_(tiers)
    host_experts, host_tiers, repaired = experts, tiers, []
    for seed in (0, 1, 2, 3):
        _, _, _, new_ref, new_err, _ = _record(H, n_tiers, seed)
        ref_d.copy_(new_ref)  # the record buffers are overwritten: the replay follows the new record ...
        err_d.copy_(new_err)
        graph.replay()
        torch.cuda.synchronize()
        # ... on the tables the replay before left in place
        want = _host(host_experts, host_tiers, n_tiers, exact, new_ref, new_err, bound)
        got_tables = _cpu(tables)
        assert got_tables[0].tolist() == want.expert_of_head.tolist() and got_tables[1].tolist() == want.tier_of_head.tolist()
        assert got_tables[3].tolist() == want.counts.tolist() and int(outs[1]) == want.repair_count
        assert outs[0].cpu().tolist()[:want.repair_count] == want.repair_list[:want.repair_count].tolist()
        assert outs[2].cpu().tolist() == want.state_of_head.tolist() and _same_floats(outs[3].cpu(), want.rel)
        for t in range(n_tiers):
            for e in range(3):
                n = int(want.counts[t, e])
                assert got_tables[2][t, e, :n].tolist() == want.lists[t, e, :n].tolist()
        host_experts, host_tiers = want.expert_of_head.to(torch.int32), want.tier_of_head.to(torch.int32)
        repaired.append(want.repair_count)
    assert repaired[0] > 0 and sum(repaired[1:]) > 0  # later records do find heads the first one kept


def test_the_registered_operator_is_the_launcher():
    import vorta_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    experts = torch.tensor(EXPERTS, dtype=torch.int32)
    H = experts.numel()
    tiers = torch.tensor([h % 2 for h in range(H)], dtype=torch.int32)
    sq_ref, sq_err = torch.tensor(SQ_REF, device=dev()), torch.tensor(SQ_ERR, device=dev())
    tables = _device_tables(experts, tiers, 2)
    got = torch.ops.vorta.route_repair(sq_ref, sq_err, *tables, 1, 0.75)
    assert len(got) == 4 and all(t.is_cuda for t in got)
    assert [(tuple(t.shape), t.dtype) for t in got] == [((H,), torch.int32), ((1,), torch.int32), ((H,), torch.int32),
                                                       ((H,), torch.float32)]
    want = _host(experts, tiers, 2, 1, SQ_REF, SQ_ERR, 0.75)
    n = want.repair_count
    assert got[0][:n].tolist() == want.repair_list[:n].tolist() and int(got[1]) == n
    assert got[2].tolist() == want.state_of_head.tolist() and _same_floats(got[3].cpu(), want.rel)
    assert tables[0].tolist() == want.expert_of_head.tolist() and tables[1].tolist() == want.tier_of_head.tolist()
    assert tables[3].tolist() == want.counts.tolist()
    one = _device_tables(experts, None, 1)
    got = torch.ops.vorta.route_repair(sq_ref, sq_err, one[0], None, one[2], one[3], 0, 0.75)  # (no tier table: one tier)
    assert got[2].tolist() == _host(experts, None, 1, 0, SQ_REF, SQ_ERR, 0.75).state_of_head.tolist()
    with FakeTensorMode():
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")  # noqa: E731
        fake = torch.ops.vorta.route_repair(torch.empty((8,), device="cuda"), torch.empty((8,), device="cuda"), i32(8), i32(8),
                                            i32(2, 3, 8), i32(2, 3), 1, 0.75)
    assert [(tuple(f.shape), f.dtype) for f in fake] == [((8,), torch.int32), ((1,), torch.int32), ((8,), torch.int32),
                                                        ((8,), torch.float32)]
    with pytest.raises(ValueError, match="vorta_route_repair"):
        torch.ops.vorta.route_repair(sq_ref, sq_err, *_device_tables(experts, tiers, 2), 2, 0.75)
