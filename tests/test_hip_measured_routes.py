"""GPU: `routed.route_by_fidelity` -- one layer routed by its own measurement, by a stated error bound or FLOP budget.

Held apart: (1) its record is `sampled_expert_fidelity(out=None)`'s on the same rows and seed, bit for bit; (2) its routes are
the host rule's, `routes_from_fidelity(record on the CPU, ..., geometry)`; (3) `routed_attention` by the returned device lists
writes the bits `routed_attention` by `HeadRouting.from_expert_ids(host table)` writes; (4) no host read, graph replay on other
q, k, v, equal bits on every run.

The bound and the share come from the record itself, so the table is mixed by construction: the bound is the midpoint between
the 2nd and 3rd smallest per-head minimum sparse error (two heads sparse, four dense); the share is half-way between the dense
layer and the layer with every head on the DEARER sparse expert (the walk moves a head, and stops before the last one).

Fixtures of tests/test_hip_routed_fidelity.py: latent (8,6,8), tile (2,3,4), window (3,3,3), coreset window (2,3,2), rate 0.5:
S = 384, H = 6; Hunyuan text 16 / 11 valid; the partial case (7,9,6) / tile (2,2,4), S = 378."""
import pytest
import torch

from test_hip_routed_fidelity import (H, P_LATENT, P_TILE, LATENT, TILE, _geom, _inputs, _text, partial_on)  # noqa: F401
from _util import dev

pytestmark = pytest.mark.gpu

N_ROWS, SEED = 96, 3
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
NAMES = ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref")


def _same_record(a, b):
    for name in NAMES:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), name
    assert a.n == b.n


def _cpu(fid):
    return fid._replace(**{name: getattr(fid, name).cpu() for name in NAMES})


def _rules(fid, geom, te):
    """a bound and a share under which the table is mixed, from the record itself"""
    from vorta_amd.patch import expert_work
    rel = fid.rel_error().cpu()[:, :2]
    best = sorted(rel.min(dim=1).values.tolist())
    assert best[1] < best[2], f"the fixture's per-head errors must be distinct: {best}"
    work = expert_work(geom, te)
    assert max(work[1:]) < work[0]
    return dict(max_rel_error=(best[1] + best[2]) / 2), dict(max_flops_share=(1 + max(work[1:]) / work[0]) / 2)


def _case(model, latent, tile, dtype):
    from vorta_amd.patch import routes_from_fidelity
    from vorta_amd.routed import HeadRouting, route_by_fidelity, routed_attention, sampled_expert_fidelity
    q, k, v, _ = _inputs(model, latent, dtype)
    T, te = _text(model)
    geom = _geom(latent, tile)
    kw = dict(model=model, text_len=T, text_valid=te)
    plain = sampled_expert_fidelity(q, k, v, geom, rows=N_ROWS, seed=SEED, **kw)
    assert bool(torch.isnan(plain.sq_err[:, 2]).all()) and bool(torch.isfinite(plain.sq_err[:, :2]).all())
    for rule in _rules(plain, geom, te):
        routing, ids, fid = route_by_fidelity(q, k, v, geom, rows=N_ROWS, seed=SEED, **rule, **kw)  # (warm)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
        try:
            routing, ids, fid = route_by_fidelity(q, k, v, geom, rows=N_ROWS, seed=SEED, **rule, **kw)
            out = routed_attention(q, k, v, routing, geom, fp8="native", **kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        _same_record(fid, plain)                                                       # (1)
        assert routing.counts_host is None and routing.counts_dev.is_cuda and ids.dtype == torch.int32 and ids.is_cuda
        table = routes_from_fidelity(_cpu(fid), rule.get("max_rel_error"), geom, te, max_flops_share=rule.get("max_flops_share"))
        print(f"{model} {latent} {dtype} {rule}: rel_error {fid.rel_error().cpu()[:, :2].tolist()} -> {table.tolist()}")
        assert ids.cpu().long().tolist() == table.tolist()                             # (2)
        assert len(set(table.tolist())) >= 2, f"a table of one expert proves nothing: {table.tolist()}"
        counts = routing.counts_dev.tolist()
        assert counts == [table.tolist().count(e) for e in range(3)]
        for e in range(3):
            assert routing.lists[e, :counts[e]].tolist() == [h for h in range(H) if int(table[h]) == e]
        want = routed_attention(q, k, v, HeadRouting.from_expert_ids(table.tolist(), dev()), geom, fp8="native", **kw)
        assert torch.equal(out, want)                                                  # (3)
        again = route_by_fidelity(q, k, v, geom, rows=N_ROWS, seed=SEED, **rule, **kw)  # the same bits on every run
        _same_record(again[2], fid)
        assert torch.equal(again[1], ids) and torch.equal(again[0].counts_dev, routing.counts_dev)
        for e in range(3):  # (entries at or past a count are not written)
            assert torch.equal(again[0].lists[e, :counts[e]], routing.lists[e, :counts[e]])
    with pytest.raises(ValueError, match="exactly one"):
        route_by_fidelity(q, k, v, geom, rows=N_ROWS, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        route_by_fidelity(q, k, v, geom, rows=N_ROWS, max_rel_error=0.1, max_flops_share=0.5, **kw)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_routes_record_and_output(model, dtype):
    _case(model, LATENT, TILE, DTYPES[dtype])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_on_a_partial_geometry(partial_on, model, dtype):
    assert _geom(P_LATENT, P_TILE).is_partial
    _case(model, P_LATENT, P_TILE, DTYPES[dtype])


@pytest.mark.parametrize("mode", ["max_rel_error", "max_flops_share"])
def test_graph_replay_on_other_inputs(mode):
    """captured on one stream with static q, k, v; other inputs are copied in; a replay gives the routes and the output of the
    eager call on those inputs"""
    from vorta_amd.routed import route_by_fidelity, routed_attention, sample_rows
    model, dtype = "hunyuan", torch.bfloat16
    T, te = _text(model)
    geom = _geom()
    first = _inputs(model, LATENT, dtype)[:3]
    gen = torch.Generator().manual_seed(99)
    second = [(x.cpu().float() * 0.5 + torch.randn(x.shape, generator=gen)).to(dtype).to(dev()) for x in first]
    kw = dict(model=model, text_len=T, text_valid=te)
    rows = sample_rows(geom.S, N_ROWS, SEED, dev())
    geom.prebuild(te)
    geom.sample_tables(te, rows)
    # one rule for both inputs, from the first: a share is mixed whatever the record; the bound is mixed on the inputs it came
    # from and is asserted on the others
    eager_first = route_by_fidelity(*first, geom, rows=rows, max_flops_share=0.5, **kw)[2]
    rule = _rules(eager_first, geom, te)[0 if mode == "max_rel_error" else 1]
    q, k, v = (x.clone() for x in first)
    out = torch.empty_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        routing, ids, fid = route_by_fidelity(q, k, v, geom, rows=rows, **rule, **kw)
        routed_attention(q, k, v, routing, geom, out=out, fp8="native", **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        routing, ids, fid = route_by_fidelity(q, k, v, geom, rows=rows, **rule, **kw)
        routed_attention(q, k, v, routing, geom, out=out, fp8="native", **kw)
    tables = []
    for inputs in (second, first):
        for dst, src in zip((q, k, v), inputs):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        e_routing, e_ids, e_fid = route_by_fidelity(*inputs, geom, rows=rows, **rule, **kw)
        want = routed_attention(*inputs, e_routing, geom, fp8="native", **kw)
        assert torch.equal(ids, e_ids) and torch.equal(routing.counts_dev, e_routing.counts_dev)
        _same_record(fid, e_fid)
        assert torch.equal(out, want)
        tables.append(ids.tolist())
    print(f"{mode}: replayed routes {tables}")
    assert len(set(tables[1])) >= 2, tables  # (the rule came from these inputs)
