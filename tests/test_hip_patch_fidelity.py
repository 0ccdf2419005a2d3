"""GPU: `vorta.patch.expert_fidelity(model)` / `fidelity_of(model)` on the mini models of tests/_mini_diffusers.py (the models,
geometry and inputs of tests/test_hip_patch_training.py), and routes derived from measured fidelity on inputs with the
structure the routed method assumes (tests/_structured_inputs.py).

1. `fidelity_of` equals, bit for bit and layer by layer, `soft_mixture_attention(..., fidelity=[...])` run again on the q, k, v
   the layer's processor launched with and that layer's routing scores; the model's output keeps its bits under the context;
   forwards outside it, and teacher forwards inside it, file nothing.
2. Structured heads: latent (8, 6, 8), tile (2, 3, 4), window (3, 3, 3), coreset window (2, 3, 2) at rate 0.5, Wan form, heads
   [local, local, redundant, redundant, white, white], noise share NOISE = 0.05, bound BOUND = 0.15 on `rel_error`.  Both were
   chosen on the CPU from the float64 oracle's own expert outputs (`oracle.routed_attention` with every head on one expert:
   what `oracle.soft_mixture_attention` mixes) so that every head sits at least a factor 2 on the right side of the bound:
       oracle rel_error (bf16-rounded inputs; fp16 agrees to the third digit)
                         coreset vs full        sliding tile vs full
       local heads       0.2734  0.2736         < 1e-4   < 1e-4          sliding <= BOUND / 2  -> sliding tile (the cheapest)
       redundant heads   0.0683  0.0640         0.5604   0.6373          coreset <= BOUND / 2, sliding >= 2 BOUND -> coreset
       white noise       1.2538  1.2113         0.5827   0.5581          both >= 2 BOUND -> full attention
   The test recomputes these ratios and checks the factor 2 before it asserts on the kernels' routes."""
import numpy as np
import pytest
import torch

import _patch_training_restate as R
import test_hip_patch_training as PT
from _util import dev

pytestmark = pytest.mark.gpu
FIELDS = ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err")
NOISE, BOUND = 0.05, 0.15
S_LATENT, S_TILE, S_WINDOW, S_GROUP = (8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)
S_HEADS = [2, 2, 1, 1, 0, 0]  # the expert whose assumption each head meets: local, local, redundant, redundant, white, white


class _SpyMixtures:
    """q, k, v (copies), geometry and keywords of every soft-mixture call (the one `routed_attention` launch with three expert
    buffers), in call order"""

    def __enter__(self):
        import vorta_amd.routed as rt
        self.rt, self.stock, self.calls = rt, rt.routed_attention, []

        def spy(q, k, v, routing, geom, **kw):
            if kw.get("expert_outs") is not None:
                self.calls.append(([x.detach().clone() for x in (q, k, v)], geom,
                                   {n: kw[n] for n in ("model", "text_len", "text_valid", "scale") if n in kw}))
            return self.stock(q, k, v, routing, geom, **kw)

        rt.routed_attention = spy
        return self

    def __exit__(self, *exc):
        self.rt.routed_attention = self.stock


def _forward(model, family, inp, **extra):
    return model(**inp, return_dict=False, self_attention_kwargs=PT._kwargs(family), **extra)[0]


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "training"])
@pytest.mark.parametrize("family,dtype", [("hunyuan", "bf16"), ("wan", "fp16")])
def test_fidelity_of_equals_the_per_layer_operator(family, dtype, grad):
    from vorta.patch import expert_fidelity, fidelity_of, original_attention, routing_scores_of
    from vorta_amd import ops
    from vorta_amd.patch._engine import context_of
    from vorta_amd.routed import soft_mixture_attention
    dt = PT.DTYPES[dtype]
    model = PT._model(family, dt)
    inp = PT._inputs(family, dt)
    n_layers = len(R.blocks_of(model))
    with pytest.raises(RuntimeError, match="expert_fidelity"):
        fidelity_of(model)
    with torch.set_grad_enabled(grad):  # (the same path: in grad mode the processors run their differentiable form)
        plain = _forward(model, family, inp).detach()
    assert context_of(model).fidelity is None  # outside the context a forward files nothing
    with torch.set_grad_enabled(grad), _SpyMixtures() as spy, expert_fidelity(model):
        if grad:
            inp = dict(inp, hidden_states=inp["hidden_states"].detach().clone().requires_grad_(True))
        out = _forward(model, family, inp)
        scores = routing_scores_of(model).detach()
    assert torch.equal(out.detach(), plain), "the model's output must keep its bits while it is measured"
    assert not context_of(model).measure_fidelity
    fid = fidelity_of(model)
    assert isinstance(fid, ops.ExpertFidelity) and len(spy.calls) == n_layers == scores.shape[0]
    H, N = spy.calls[0][0][0].shape[-3], spy.calls[0][0][0].shape[-2]
    assert fid.sq_ref.shape == fid.max_ref.shape == (n_layers, H) and fid.sq_err.shape == fid.max_err.shape == (n_layers, H, 3)
    assert fid.n == N * 128 and fid.rel_error().shape == (n_layers, H, 3)
    assert bool(torch.isfinite(fid.rel_error()).all()) and bool((fid.rel_error()[..., :2] > 0).all())
    for layer, ((q, k, v), geom, kw) in enumerate(spy.calls):
        again = []
        soft_mixture_attention(q, k, v, scores[layer], geom, fidelity=again, **kw)
        for name in FIELDS:
            assert torch.equal(getattr(fid, name)[layer], getattr(again[0], name)), (layer, name)
    if grad:  # the statistics are no part of the graph: the training step goes on
        out.float().sum().backward()
        assert inp["hidden_states"].grad is not None and bool(torch.isfinite(inp["hidden_states"].grad).all())
    # a teacher forward inside the context measures nothing and leaves the record alone; a forward outside it too
    with torch.no_grad(), expert_fidelity(model), original_attention(model):
        model(**PT._inputs(family, dt), return_dict=False)
    with torch.no_grad():
        _forward(model, family, PT._inputs(family, dt))
    later = fidelity_of(model)
    assert all(torch.equal(getattr(later, n), getattr(fid, n)) for n in FIELDS)


def _oracle_rel_errors(q, k, v):
    """(H, 2) rel_error of the coreset and the sliding-tile expert against full attention, by the float64 oracle"""
    from oracle import vorta_oracle as O
    f64 = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    gi = O.group_info(S_LATENT, S_GROUP, 0.5)
    H = q.shape[1]
    outs = [O.routed_attention(f64(q), f64(k), f64(v), np.full(H, e, dtype=np.int32), model="wan", latent=S_LATENT,
                               tile=S_TILE, window=S_WINDOW, gi=gi) for e in range(3)]
    ref = (outs[0] ** 2).sum((0, 2, 3))
    return np.stack([np.sqrt(((outs[e] - outs[0]) ** 2).sum((0, 2, 3)) / ref) for e in (1, 2)], axis=1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_routes_from_measured_fidelity_on_structured_heads(dtype):
    import _structured_inputs as SI
    from vorta.patch import evaluate_routing, routes_from_fidelity
    from vorta.patch.fidelity import stack_fidelity
    from vorta_amd.routed import geometry_for, soft_mixture_attention
    dt = PT.DTYPES[dtype]
    gen = torch.Generator().manual_seed(1234)
    q, k, v = (x.to(dt) for x in SI.structured_layer(S_LATENT, S_HEADS, S_TILE, S_GROUP, NOISE, gen, "cpu"))
    # the premise, from the oracle alone: every head a factor 2 on the right side of the bound
    rel = _oracle_rel_errors(q, k, v)
    print(f"oracle rel_error ({dtype}; coreset, sliding tile per head):\n{np.round(rel, 4)}")
    for h, kind in enumerate(S_HEADS):
        if kind == 2:
            assert rel[h, 1] <= BOUND / 2, (h, rel[h])
        elif kind == 1:
            assert rel[h, 0] <= BOUND / 2 and rel[h, 1] >= 2 * BOUND, (h, rel[h])
        else:
            assert rel[h, 0] >= 2 * BOUND and rel[h, 1] >= 2 * BOUND, (h, rel[h])
    geom = geometry_for(S_LATENT, S_TILE, S_WINDOW, S_GROUP, 0.5, dev())
    sc = torch.full((1, len(S_HEADS), 3), 1.0 / 3.0, device=dev())
    filed = []
    soft_mixture_attention(*(x.to(dev()) for x in (q, k, v)), sc, geom, model="wan", fidelity=filed)
    fid = stack_fidelity(filed)  # one layer
    got = fid.rel_error()[0, :, :2].cpu().numpy()
    print(f"kernel rel_error ({dtype}):\n{np.round(got, 4)}")
    table = routes_from_fidelity(fid, BOUND)
    assert table.tolist() == [S_HEADS]  # local -> sliding tile, redundant -> coreset, white noise -> full
    assert routes_from_fidelity(fid, BOUND, geometry=geom).tolist() == [S_HEADS]
    # what these routes cost and lose, and what all-sparse routes would lose
    r = evaluate_routing(table, fid, geom)
    assert float(r["worst_rel_error"][0]) <= BOUND and 0.0 < float(r["flops_share"][0]) < 1.0
    bad = evaluate_routing(torch.full((1, len(S_HEADS)), 2), fid, geom)
    assert float(bad["worst_rel_error"][0]) >= 2 * BOUND
