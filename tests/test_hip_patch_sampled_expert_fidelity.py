"""GPU: `vorta.patch.sampled_expert_fidelity(model)` / `sampled_expert_fidelity_of(model)` / `fixed_routes(model, table)` on the
hard-routing (Eval) mini models of tests/_mini_diffusers.py (the models, geometry and inputs of tests/test_hip_patch.py: latent
(4,6,8), S = 192, 16 / 11 text).

The loop the feature exists for: measure every expert of every head on sampled rows -> `routes_from_fidelity(fid, b)` -> run the
same forward by that table -> `routed_fidelity` reports the table as launched and, for every sparse head, the error the
counterfactual column promised.

Which counterfactual.  A table that differs from the first forward's routes changes layer 0's output and so the q, k, v of every
later layer: the first forward's columns promise something for LAYER 0 only, whose inputs do not depend on any route.  There the
measured error equals the first forward's column and is within the bound.  For every layer the table-routed forward is measured
by both contexts at once, and a sparse head's measured error equals the counterfactual column of that same forward.

How "equals" is held.  The two records come from two reductions of the SAME rows (vorta_expert_fidelity: 64 parts a head;
vorta_sampled_fidelity: 16), so the sums of squares agree to their chains of float32 roundings, not to the bit:
|rel - rel'| <= (VORTA_FIDELITY_CHAIN(n) + VORTA_SAMPLED_FIDELITY_CHAIN(n) + 4) 2^-24 relative (each sum within its chain, twice
-- numerator and denominator -- halved by the square root; + 4 for the two divisions and roots).  The maxima are exact in both
kernels: `max_err` and `max_ref` are compared bit for bit, which only the same rows give.  And inside one kernel the match IS
exact: the record of the table-routed forward has column 2 (the routed output) equal to the launched expert's column."""
import pytest
import torch

import test_hip_patch as TP
from _util import dev

pytestmark = pytest.mark.gpu
N_ROWS, SEED = 64, 3
# a tile sees its own tile only: with test_hip_patch's window (3,3,3) every tile of this latent sees every tile, the sliding
# expert is full attention in another summation order (rel_error 7e-4) and no single bound leaves all three experts
WINDOW = (1, 1, 1)
# the bound of `routes_from_fidelity`: inside a gap of the fixture's measured errors (the test prints them) -- Hunyuan: sliding
# 0.37 - 0.59, coreset 0.31 - 0.41, the bound between 0.3852 and 0.4104; Wan: sliding 0.29 - 0.42, coreset 0.29 - 0.47, the
# bound between 0.3437 and 0.3514, which also leaves layer 0 one head on each expert -- so that the table holds all three experts:
# asserted on the run itself
BOUND = {"hunyuan": 0.398, "wan": 0.3475}


def _kwargs(family):
    from vorta.patch.utils import prepare_hunyuan_self_attn_kwargs, prepare_wan_self_attn_kwargs
    prepare = prepare_hunyuan_self_attn_kwargs if family == "hunyuan" else prepare_wan_self_attn_kwargs
    return prepare(dict(latent_shape=TP.LATENT, window_size=WINDOW, tile_size=TP.TILE, lowres_window_size=TP.GROUP,
                        lowres_reduction_rate=0.5), dev(), TP.TAU)


def _setup(family):
    if family == "hunyuan":
        return TP._hy_model(), TP._hy_inputs, lambda: _kwargs("hunyuan")
    return TP._wan_model(), TP._wan_inputs, lambda: _kwargs("wan")


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_measure_then_route_by_the_table(family):
    from vorta.patch import (evaluate_routing, fixed_routes, routed_fidelity, routed_fidelity_of, routes_from_fidelity,
                             sampled_expert_fidelity, sampled_expert_fidelity_of)
    from vorta_amd import _C, ops
    from vorta_amd.patch._engine import context_of
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    forward = lambda kw=None: model(**inputs(), return_dict=False, self_attention_kwargs=kw or kwargs())[0]  # noqa: E731
    with pytest.raises(RuntimeError, match="sampled_expert_fidelity"):
        sampled_expert_fidelity_of(model)
    with torch.no_grad():
        plain = forward()
        with sampled_expert_fidelity(model, n_rows=N_ROWS, seed=SEED):
            out = forward()
    assert torch.equal(out, plain), "the model's output must keep its bits while it is measured"
    assert ctx.measure_experts is None and ctx.routed_fidelity is None
    fid = sampled_expert_fidelity_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    assert isinstance(fid, ops.ExpertFidelity) and fid.n == N_ROWS * 128
    assert fid.sq_ref.shape == (L, H) and fid.sq_err.shape == (L, H, 3) and bool(torch.isfinite(fid.sq_err).all())
    rel = fid.rel_error().cpu()
    print(f"{family}: counterfactual rel_error (layer, head, [coreset, sliding, routed])\n{rel}")
    b = BOUND[family]
    table = routes_from_fidelity(fid, b, kwargs())  # (the cost order of THIS geometry: expert_work)
    print(f"{family}: errors in order {sorted(rel[..., :2].flatten().tolist())}\ntable\n{table}")
    assert sorted(set(table.flatten().tolist())) == [0, 1, 2], f"the bound {b} must leave all three experts in the table: {table}"
    with torch.no_grad(), fixed_routes(model, table), routed_fidelity(model, n_rows=N_ROWS, seed=SEED, heads="all"), \
            sampled_expert_fidelity(model, n_rows=N_ROWS, seed=SEED):
        routed = forward()
        kw = kwargs()
        kw.pop("tau_sparse")
        assert torch.equal(forward(kw), routed), "tau_sparse is not consulted under fixed_routes"
    rf, fid2 = routed_fidelity_of(model), sampled_expert_fidelity_of(model)
    assert torch.equal(rf.expert.cpu().long(), table), "the launches must follow the table"
    assert torch.equal(fid2.sq_err[0, :, :2], fid.sq_err[0, :, :2]) and torch.equal(fid2.sq_ref[0], fid.sq_ref[0])  # layer 0: same q, k, v
    assert torch.equal(rf.max_ref, fid2.max_ref)
    got, rel2 = rf.rel_error().cpu(), fid2.rel_error().cpu()
    assert any(int(e) != 0 for e in table[0]), "layer 0 must hold a sparse head"
    tol = (_C.fidelity_chain(N_ROWS) + _C.sampled_fidelity_chain(N_ROWS) + 4) * 2.0 ** -24
    sparse = 0
    for layer in range(L):
        for h in range(H):
            e = int(table[layer, h])
            if e == 0:
                assert float(fid2.sq_err[layer, h, 2]) == 0.0  # a full-attention head in the input dtype: the dense rows
                continue
            sparse += 1
            want = float(rel2[layer, h, e - 1])
            assert float(fid2.sq_err[layer, h, 2]) == float(fid2.sq_err[layer, h, e - 1])
            assert float(rf.max_err[layer, h]) == float(fid2.max_err[layer, h, e - 1])
            assert abs(float(got[layer, h]) - want) <= tol * want, (layer, h, e, float(got[layer, h]), want)
            if layer == 0:  # the column the table was built from
                assert want == float(rel[0, h, e - 1]) and float(got[0, h]) <= b and want <= b
    assert sparse > 0
    r = evaluate_routing(rf.expert, rf, kwargs())
    print(f"{family}: table {table.tolist()}, measured under it {got.tolist()}, worst per layer {r['worst_rel_error'].tolist()}")
    assert float(r["worst_rel_error"][0]) <= b
    with torch.no_grad():
        assert torch.equal(forward(), plain), "outside the context nothing changes"
    assert ctx.fixed_routes is None


def test_fixed_routes_refuses_a_bad_table_and_the_contexts_share_one_sample():
    from vorta.patch import fixed_routes, routed_fidelity, sampled_expert_fidelity
    from vorta_amd.patch._engine import context_of
    model, _, _ = _setup("wan")
    L, H = len(context_of(model).plan), context_of(model).plan.heads
    for bad in (torch.zeros((L, H + 1), dtype=torch.int64), torch.zeros((L,), dtype=torch.int64),
                torch.full((L, H), 3), torch.full((L, H), -1), torch.zeros((L, H))):
        with pytest.raises(ValueError, match="fixed_routes"):
            with fixed_routes(model, bad):
                pass
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        with fixed_routes(torch.nn.Linear(2, 2), torch.zeros((1, 1), dtype=torch.int64)):
            pass
    with pytest.raises(ValueError, match="share one sample"):
        with routed_fidelity(model, n_rows=32, seed=0), sampled_expert_fidelity(model, n_rows=64, seed=0):
            pass
    with pytest.raises(ValueError, match="share one sample"):
        with sampled_expert_fidelity(model, n_rows=32, seed=1), routed_fidelity(model, n_rows=32, seed=0):
            pass
    assert context_of(model).measure_experts is None and context_of(model).measure_routed is None
