"""GPU: `ops.route_fidelity` (vorta_route_fidelity) against the host rule, `vorta.patch.routes_from_fidelity`, which is the
definition.  The host rule is always evaluated on CPU copies of the record; the table, the counts, the listed heads and the
FLOP share must be EQUAL -- there is no tolerance: the relative error is two correctly rounded float32 operations and the cost
a handful of double ones, from integer counts.

A crafted H = 7 record (a tie exactly at the bound, NaN, inf, both sq_ref == 0 cases, a head both experts qualify for, under
three work vectors); random records with errors from a small set, so that ties are common, at H in {1, 6, 24, 40, 1024};
the error codes; a graph replay on other statistics."""
import ctypes as C

import pytest
import torch

from _util import dev

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SEEDS = 200
# sums of squares whose ratios are squares of short binary fractions: rel lands on 0.25, 0.5, 0.75, 1, ... exactly, again and again
SQ_REF = [0.0, 1.0, 4.0, 16.0, 16.0, 16.0]
SQ_ERR = [0.0, 0.25, 1.0, 1.0, 4.0, 9.0, 9.0, 16.0, 3.0, 1e-30, NAN, INF]
WORKS = [(3.0, 2.0, 1.0), (3.0, 1.0, 2.0), (3.0, 2.0, 2.0), (5.0, 5.0, 1.5), (4.0, 6.0, 1.0), (2.0, 3.0, 2.0),
         (1.2176e15, 3.1e14, 2.9e14), (0.7, 0.1, 0.3)]
BOUNDS = [0.0, 0.25, 0.5, 0.75, 1.0, 0.4330127, 3.0, INF]
SHARES = [0.01, 0.3, 0.5, 0.625, 0.75, 0.9, 1.0, 2.0]


def _fid(sq_ref, sq_err, device=None):
    from vorta_amd.ops import ExpertFidelity
    sq_ref, sq_err = (torch.as_tensor(x, dtype=torch.float32) for x in (sq_ref, sq_err))
    if device is not None:
        sq_ref, sq_err = sq_ref.to(device), sq_err.to(device)
    return ExpertFidelity(sq_ref, sq_ref.sqrt(), sq_err, sq_err.sqrt(), None, 128)


def _record(H, seed):
    g = torch.Generator().manual_seed(1000 * H + seed)
    pick = lambda values, shape: torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]  # noqa: E731
    choose = lambda values: values[int(torch.randint(0, len(values), (1,), generator=g))]  # noqa: E731
    sq_err = pick(SQ_ERR, (H, 3))
    sq_err[:, 2] = NAN  # the routed column of a measurement without `out`: never read
    return pick(SQ_REF, (H,)), sq_err, choose(WORKS), choose(BOUNDS), choose(SHARES)


def _host(sq_ref, sq_err, work, **rule):
    from vorta_amd.patch import routes_from_fidelity
    return routes_from_fidelity(_fid(sq_ref.cpu(), sq_err.cpu()), rule.get("max_rel_error"), dict(work=work),
                                max_flops_share=rule.get("max_flops_share")).tolist()


def _check(got, want, work, case):
    """one call's device outputs (already on the host) against the host table"""
    expert, lists, counts, share = got
    H = len(want)
    assert expert == want, f"{case}: expert table {expert} != host {want}"
    heads = [[h for h in range(H) if want[h] == e] for e in range(3)]
    assert counts == [len(x) for x in heads], f"{case}: counts {counts}"
    for e in range(3):
        assert lists[e][:counts[e]] == heads[e], f"{case}: list of expert {e}"
    n = counts
    formula = (n[0] * work[0] + n[1] * work[1] + n[2] * work[2]) / (H * work[0])
    assert share == float(torch.tensor(formula, dtype=torch.float64).float()), f"{case}: share {share} != {formula}"


CRAFTED_REF = [16.0, 1.0, 1.0, 0.0, 0.0, 16.0, 16.0]
CRAFTED_ERR = [[9.0, 100.0, NAN],    # coreset exactly AT the bound 0.75: it qualifies
               [NAN, NAN, NAN],       # NaN meets no bound
               [INF, INF, NAN],       # inf
               [0.0, 0.0, NAN],       # sq_ref == 0 and sq_err == 0: rel 0, both qualify
               [1.0, 2.0, NAN],       # sq_ref == 0 and sq_err > 0: inf
               [1.0, 4.0, NAN],       # 0.25 and 0.5: both qualify
               [16.0, 25.0, NAN]]     # 1 and 1.25: neither


@pytest.mark.parametrize("work, want", [((3.0, 2.0, 1.0), [1, 0, 0, 2, 0, 2, 0]),     # sliding tile cheaper
                                        ((3.0, 1.0, 2.0), [1, 0, 0, 1, 0, 1, 0]),     # coreset cheaper
                                        ((3.0, 2.0, 2.0), [1, 0, 0, 2, 0, 2, 0])])    # equal work: expert 2
def test_crafted_record_under_an_error_bound(work, want):
    from vorta_amd import ops
    fid = _fid(CRAFTED_REF, CRAFTED_ERR, dev())
    got = ops.route_fidelity(fid, max_rel_error=0.75, work=work, flops_share=True)
    assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32] * 3 + [torch.float32]
    assert _host(fid.sq_ref, fid.sq_err, work, max_rel_error=0.75) == want
    _check([t.cpu().tolist() for t in got[:3]] + [float(got[3])], want, work, f"crafted {work}")
    if work == (3.0, 2.0, 1.0):  # work=None is that order
        assert ops.route_fidelity(fid, max_rel_error=0.75)[0].tolist() == want
    # just under the bound the tie is out
    below = ops.route_fidelity(fid, max_rel_error=0.7499999, work=work)[0].tolist()
    assert below == [0] + want[1:] == _host(fid.sq_ref, fid.sq_err, work, max_rel_error=0.7499999)


@pytest.mark.parametrize("work", WORKS[:3])
def test_crafted_record_under_a_budget(work):
    from vorta_amd import ops
    fid = _fid(CRAFTED_REF, CRAFTED_ERR, dev())
    seen = set()
    for share in (0.99, 0.95, 0.9, 0.85, 0.8, 0.7, 0.5, 0.01):
        want = _host(fid.sq_ref, fid.sq_err, work, max_flops_share=share)
        got = ops.route_fidelity(fid, max_flops_share=share, work=work, flops_share=True)
        _check([t.cpu().tolist() for t in got[:3]] + [float(got[3])], want, work, f"crafted {work} share {share}")
        seen.add(tuple(want))
    # the ranking: head 3 (rel 0), head 5 (0.25), head 0 (0.75); heads 1, 2, 4 have no candidate; head 6 (1.0) is last
    assert _host(fid.sq_ref, fid.sq_err, work, max_flops_share=0.99) == [0, 0, 0, 2 if work[2] <= work[1] else 1, 0, 0, 0]
    assert [x != 0 for x in _host(fid.sq_ref, fid.sq_err, work, max_flops_share=0.01)] == [True, False, False, True, False, True, True]
    assert len(seen) >= 4


@pytest.mark.parametrize("mode", ["max_rel_error", "max_flops_share"])
@pytest.mark.parametrize("H", [1, 6, 24, 40, 1024])
def test_random_records_equal_the_host_rule(H, mode):
    from vorta_amd import ops
    cases, outs = [], []
    for seed in range(SEEDS):
        sq_ref, sq_err, work, bound, share = _record(H, seed)
        rule = {mode: bound if mode == "max_rel_error" else share}
        cases.append((sq_ref, sq_err, work, rule))
        outs.append(ops.route_fidelity(_fid(sq_ref, sq_err, dev()), work=work, flops_share=True, **rule))
    torch.cuda.synchronize()
    tables = set()
    for seed, ((sq_ref, sq_err, work, rule), got) in enumerate(zip(cases, outs)):
        want = _host(sq_ref, sq_err, work, **rule)
        _check([t.cpu().tolist() for t in got[:3]] + [float(got[3])], want, work, f"H={H} seed={seed} {rule} work={work}")
        tables.add(tuple(want))
    assert len(tables) >= (2 if H == 1 else 20)  # the draws do exercise the rule


def _raw_args(fid, expert, lists, counts, **kw):
    from vorta_amd import _C
    a = _C.RouteFidelityArgs()
    a.struct_size, a.heads, a.mode, a.max_rel_error, a.max_flops_share = C.sizeof(a), fid.sq_ref.numel(), 0, 0.75, 0.5
    a.sq_ref, a.sq_err = fid.sq_ref.data_ptr(), fid.sq_err.data_ptr()
    a.expert_of_head, a.head_lists, a.head_counts = expert.data_ptr(), lists.data_ptr(), counts.data_ptr()
    a.work[0], a.work[1], a.work[2] = 3.0, 2.0, 1.0
    for key, value in kw.items():
        setattr(a, key, value)
    return a


def test_error_codes_and_nothing_is_launched():
    from vorta_amd import _C, ops
    fid = _fid(CRAFTED_REF, CRAFTED_ERR, dev())
    outs = [torch.full(shape, -7, dtype=torch.int32, device=dev()) for shape in ((7,), (3, 7), (3,))]
    lib, stream = _C.lib(), torch.cuda.current_stream().cuda_stream
    bad = [dict(heads=1025), dict(heads=0), dict(sq_ref=None), dict(head_counts=None), dict(max_rel_error=-0.5),
           dict(max_rel_error=NAN), dict(mode=1, max_flops_share=0.0), dict(mode=1, max_flops_share=NAN), dict(mode=2),
           dict(struct_size=C.sizeof(_C.RouteFidelityArgs) - 8)]
    for kw in bad:
        assert lib.vorta_route_fidelity(C.byref(_raw_args(fid, *outs, **kw)), stream) == _C.VORTA_EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call wrote its outputs"
    assert lib.vorta_route_fidelity(C.byref(_raw_args(fid, *outs)), stream) == _C.VORTA_OK  # the same block, unspoilt
    assert outs[0].tolist() == [1, 0, 0, 2, 0, 2, 0] and outs[2].tolist() == [4, 1, 2]
    assert outs[1][0, :4].tolist() == [1, 2, 4, 6] and outs[1][0, 4:].tolist() == [-7] * 3  # past the count: not written
    big = _fid([1.0] * 1025, [[0.0, 0.0, NAN]] * 1025, dev())
    with pytest.raises(ValueError, match="vorta_route_fidelity"):
        ops.route_fidelity(big, max_rel_error=0.5)
    with pytest.raises(ValueError, match="vorta_route_fidelity"):
        ops.route_fidelity(fid, max_rel_error=-1.0)
    with pytest.raises(ValueError, match="vorta_route_fidelity"):
        ops.route_fidelity(fid, max_flops_share=0.0)
    with pytest.raises(ValueError, match="vorta_route_fidelity"):
        ops.route_fidelity(fid, max_rel_error=0.5, work=(3.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="exactly one"):
        ops.route_fidelity(fid, max_rel_error=0.5, max_flops_share=0.5)
    with pytest.raises(ValueError, match="ONE layer"):
        ops.route_fidelity(_fid([CRAFTED_REF], [CRAFTED_ERR], dev()), max_rel_error=0.5)


@pytest.mark.parametrize("mode", ["max_rel_error", "max_flops_share"])
def test_graph_replay_follows_the_statistics_in_the_buffers(mode):
    from vorta_amd import ops
    H = 40
    sq_ref, sq_err, work, _, _ = _record(H, 0)
    rule = {mode: 0.5}
    static = _fid(sq_ref, sq_err, dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        ops.route_fidelity(static, work=work, flops_share=True, **rule)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.route_fidelity(static, work=work, flops_share=True, **rule)
    tables = set()
    for seed in (0, 1, 2, 3):
        new_ref, new_err = _record(H, seed)[:2]
        static.sq_ref.copy_(new_ref)
        static.sq_err.copy_(new_err)
        graph.replay()
        torch.cuda.synchronize()
        want = _host(new_ref, new_err, work, **rule)
        _check([t.cpu().tolist() for t in got[:3]] + [float(got[3])], want, work, f"replay {mode} seed {seed}")
        tables.add(tuple(want))
    assert len(tables) == 4
    # the same bits on every run
    again = ops.route_fidelity(static, work=work, flops_share=True, **rule)
    _check([t.cpu().tolist() for t in again[:3]] + [float(again[3])], want, work, f"eager after the replays {mode}")
    assert all(torch.equal(again[i], got[i]) for i in (0, 2, 3))  # (the lists: up to their counts, checked above)


@pytest.mark.parametrize("rule", [dict(max_rel_error=0.75), dict(max_flops_share=0.8)])
def test_the_registered_operator_is_the_launcher(rule):
    """torch.ops.vorta.route_fidelity: its four outputs are ops.route_fidelity(..., flops_share=True)'s, and its shape function
    gives their shapes and dtypes"""
    import vorta_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vorta_amd import ops
    fid = _fid(CRAFTED_REF, CRAFTED_ERR, dev())
    work = [3.0, 1.0, 2.0]
    want = ops.route_fidelity(fid, work=work, flops_share=True, **rule)
    got = torch.ops.vorta.route_fidelity(fid.sq_ref, fid.sq_err, work=work, **rule)
    assert len(got) == 4
    counts = want[2].tolist()
    for name, a, b in zip(("expert", "lists", "counts", "share"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_cuda, name
        if name == "lists":  # (entries at or past a count are not written)
            assert all(torch.equal(a[e, :counts[e]], b[e, :counts[e]]) for e in range(3))
        else:
            assert torch.equal(a, b), name
    _check([t.cpu().tolist() for t in got[:3]] + [float(got[3])], _host(fid.sq_ref, fid.sq_err, tuple(work), **rule), work, "operator")
    default = torch.ops.vorta.route_fidelity(fid.sq_ref, fid.sq_err, max_rel_error=0.75)  # work=None: (3, 2, 1)
    assert default[0].tolist() == [1, 0, 0, 2, 0, 2, 0]
    with FakeTensorMode():
        fake = torch.ops.vorta.route_fidelity(torch.empty((7,), device="cuda"), torch.empty((7, 3), device="cuda"), work=work, **rule)
    assert [(tuple(f.shape), f.dtype) for f in fake] == [(tuple(t.shape), t.dtype) for t in want]
    with pytest.raises(ValueError, match="exactly one"):
        torch.ops.vorta.route_fidelity(fid.sq_ref, fid.sq_err)
