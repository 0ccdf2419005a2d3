"""GPU: `vorta.patch.routed_fidelity(model)` / `routed_fidelity_of(model)` on the hard-routing (Eval) mini models of
tests/_mini_diffusers.py (the models, geometry and inputs of tests/test_hip_patch.py: latent (4,6,8), S = 192, 16 / 11 text).

`routed_fidelity_of` equals, bit for bit and layer by layer, `routed_attention(..., fidelity=[...])` run again on the q, k, v and
the head lists the layer's processor launched with; the model's output keeps its bits under the context; forwards outside it,
and teacher forwards inside it, launch what they launch today and file nothing; `expert_fidelity` still measures nothing on an
Eval model; `evaluate_routing` takes the sampled record."""
import pytest
import torch

import test_hip_patch as TP
from _sampled_fidelity_restate import NAMES
from _util import dev

pytestmark = pytest.mark.gpu
N_ROWS, SEED = 32, 3


class _Launches:
    """every `routed.routed_attention` call (inputs cloned, geometry, keywords) and every `ops.sampled_fidelity` call"""

    def __enter__(self):
        import vorta_amd.routed as rt
        from vorta_amd import ops
        self.rt, self.ops, self.stock, self.stock_cmp = rt, ops, rt.routed_attention, ops.sampled_fidelity
        self.calls, self.compares = [], 0

        def routed(q, k, v, routing, geom, **kw):
            self.calls.append(dict(qkv=[x.detach().clone() for x in (q, k, v)], lists=routing.lists.clone(),
                                   counts=routing.counts_dev.clone(), geom=geom, kw=dict(kw)))
            return self.stock(q, k, v, routing, geom, **kw)

        def compare(*a, **kw):
            self.compares += 1
            return self.stock_cmp(*a, **kw)

        rt.routed_attention, ops.sampled_fidelity = routed, compare
        return self

    def __exit__(self, *exc):
        self.rt.routed_attention, self.ops.sampled_fidelity = self.stock, self.stock_cmp


def _setup(family):
    if family == "hunyuan":
        return TP._hy_model(), TP._hy_inputs, TP._hy_kwargs
    return TP._wan_model(), TP._wan_inputs, TP._wan_kwargs


@pytest.mark.parametrize("heads", ["sparse", "all"])
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_routed_fidelity_of_equals_the_per_layer_operator(family, heads):
    from vorta.patch import (evaluate_routing, expert_fidelity, fidelity_of, original_attention, routed_fidelity,
                             routed_fidelity_of)
    from vorta_amd import ops
    from vorta_amd.patch._engine import context_of
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    forward = lambda **extra: model(**inputs(), return_dict=False, self_attention_kwargs=kwargs(), **extra)[0]  # noqa: E731
    with pytest.raises(RuntimeError, match="routed_fidelity"):
        routed_fidelity_of(model)
    with torch.no_grad(), _Launches() as before:
        plain = forward()
    assert ctx.routed_fidelity is None and before.compares == 0
    assert all(not any(name.startswith("fidelity") for name in c["kw"]) for c in before.calls)  # today's launches
    with torch.no_grad(), _Launches() as rec, routed_fidelity(model, n_rows=N_ROWS, seed=SEED, heads=heads):
        out = forward()
    assert torch.equal(out, plain), "the model's output must keep its bits while it is measured"
    assert ctx.measure_routed is None and len(rec.calls) == len(before.calls) > 1
    rf = routed_fidelity_of(model)
    L, H = len(rec.calls), rec.calls[0]["qkv"][0].shape[-3]
    assert isinstance(rf, ops.SampledFidelity) and rf.n == N_ROWS * 128
    assert all(getattr(rf, name).shape == (L, H) for name in NAMES) and rf.expert.shape == (L, H)
    tokens = sample_rows(TP.S, N_ROWS, SEED, dev())
    assert torch.equal(rf.rows, tokens)
    for layer, c in enumerate(rec.calls):
        assert torch.equal(c["kw"]["fidelity_rows"], tokens) and c["kw"]["fidelity_heads"] == heads
        again = []
        kw = {n: c["kw"][n] for n in ("model", "text_len", "text_valid") if n in c["kw"]}
        routed_attention(*c["qkv"], HeadRouting.from_device(c["lists"], c["counts"]), c["geom"], fidelity=again,
                         fidelity_rows=tokens, fidelity_heads=heads, **kw)
        for name in NAMES:
            a, b = getattr(rf, name)[layer], getattr(again[0], name)
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num()), (layer, name)
        experts = TP._experts_from(dict(lists=c["lists"], counts=c["counts"]), H)
        assert rf.expert[layer].tolist() == experts.tolist()
        measured = [h for h in range(H) if heads == "all" or experts[h] != 0]
        assert torch.isfinite(rf.sq_err[layer]).nonzero().flatten().tolist() == measured
    assert len({tuple(x) for x in rf.expert.tolist()}) > 1  # layers that disagree: every layer got its own routes
    # the sampled record in evaluate_routing: a head's error is its measured one
    rel = rf.rel_error().cpu()
    r = evaluate_routing(rf.expert, rf, kwargs())
    want = torch.where(torch.isnan(rel), torch.zeros_like(rel), rel)  # (an unmeasured head is a full-attention head here: 0)
    assert torch.equal(r["worst_rel_error"], want.max(-1).values) and torch.equal(r["mean_rel_error"], want.mean(-1))
    assert r["experts"].tolist() == rf.expert.tolist() and bool((r["flops_share"] > 0).all())
    other = (rf.expert.cpu().long() + 1) % 3
    with pytest.raises(ValueError, match="launched"):
        evaluate_routing(other, rf, kwargs())
    # a teacher forward inside the context measures nothing and leaves the record alone; a forward outside it too
    # (the teacher pass of the Hunyuan form: Wan's hard-routing processor serves `original_attention` through its Train form only)
    if family == "hunyuan":
        with torch.no_grad(), _Launches() as quiet, routed_fidelity(model, n_rows=N_ROWS), original_attention(model):
            model(**inputs(), return_dict=False)
        assert quiet.compares == 0 and not quiet.calls
    with torch.no_grad(), _Launches() as quiet2:
        forward()
    assert quiet2.compares == 0
    later = routed_fidelity_of(model)
    assert all(torch.equal(getattr(later, n).nan_to_num(), getattr(rf, n).nan_to_num()) for n in NAMES)
    # the soft mixture's context on an Eval model still measures nothing, of either kind
    with torch.no_grad(), _Launches() as soft, expert_fidelity(model):
        assert torch.equal(forward(), plain)
    assert soft.compares == 0 and ctx.fidelity is None
    assert all(not any(name.startswith("fidelity") for name in c["kw"]) for c in soft.calls)
    with pytest.raises(RuntimeError, match="expert_fidelity"):
        fidelity_of(model)


def test_default_sample_covers_a_small_clip_and_bad_arguments_are_refused():
    from vorta.patch import routed_fidelity, routed_fidelity_of
    model, inputs, kwargs = _setup("wan")
    with torch.no_grad(), routed_fidelity(model):  # n_rows = 2048 > S = 192: every row
        model(**inputs(), return_dict=False, self_attention_kwargs=kwargs())
    rf = routed_fidelity_of(model)
    assert rf.rows.tolist() == list(range(TP.S)) and rf.n == TP.S * 128
    with pytest.raises(ValueError):
        with routed_fidelity(model, heads="dense"):
            pass
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        with routed_fidelity(torch.nn.Linear(2, 2)):
            pass


def test_latent_shape_left_to_the_processors_default(monkeypatch):
    """a caller whose self_attention_kwargs do not name `latent_shape` runs the processor's own default; the measured path sizes
    its sample from the same default (here the default is set to the mini model's latent, which the plain forward needs too)"""
    import inspect
    from vorta.patch import routed_fidelity, routed_fidelity_of
    from vorta_amd.patch._engine import context_of
    model, inputs, kwargs = _setup("wan")
    kw = kwargs()
    latent = tuple(int(x) for x in kw.pop("latent_shape"))
    wrappers = [m.processor for m in model.modules() if getattr(getattr(m, "processor", None), "_default_latent", None) is not None]
    assert wrappers and all(w._default_latent == inspect.signature(w.inner.__call__).parameters["latent_shape"].default
                            for w in wrappers)
    call = type(wrappers[0].inner).__call__
    monkeypatch.setattr(type(wrappers[0].inner), "__call__",
                        lambda self, *a, **k: call(self, *a, **dict(dict(latent_shape=latent), **k)))
    for w in wrappers:
        monkeypatch.setattr(w, "_default_latent", latent)
    with torch.no_grad():
        plain = model(**inputs(), return_dict=False, self_attention_kwargs=dict(kw))[0]
    with torch.no_grad(), routed_fidelity(model, n_rows=N_ROWS, seed=SEED):
        out = model(**inputs(), return_dict=False, self_attention_kwargs=dict(kw))[0]
    assert torch.equal(out, plain)
    rf = routed_fidelity_of(model)
    assert rf.rows.numel() == N_ROWS and int(rf.rows.max()) < TP.S and context_of(model).measure_routed is None
