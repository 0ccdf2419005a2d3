"""CPU: router training through the patched transformers (vorta_amd/patch/_engine.py) up to the GPU boundary.

The mini models of tests/_mini_diffusers.py are patched with `train_router=True, differentiable=True`; every attention
processor behind a `BoundProcessor` is then replaced by a stub that records what it is handed and returns a torch
expression of it, so no kernel is needed: which scores reach which layer, whether they carry a graph, and which forward's
state a block sees when gradient checkpointing recomputes it after other forwards have run."""
import gc
import inspect
import weakref

import pytest
import torch
from torch.utils.checkpoint import checkpoint

import _mini_diffusers as M

KW = dict(latent_shape=(4, 6, 8), window_size=(3, 3, 3), tile_size=(2, 3, 4), lowres_window_size=(2, 3, 2),
          lowres_reduction_rate=0.5)
BF = torch.bfloat16


class _Stub:
    """stands where a Train processor stood: same keywords, a differentiable stand-in for the attention"""
    differentiable = True

    def __init__(self, log, layer):
        self.log, self.layer = log, layer

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask, rotary, use_original_attn=False,
                 routing_score=None, lowres_group_info=None, flex_attn_mask_func=None, window_size=None, tile_size=None,
                 latent_shape=None):
        self.log.append(dict(layer=self.layer, teacher=use_original_attn, score=routing_score, group=lowres_group_info,
                             descriptor=flex_attn_mask_func, grad_mode=torch.is_grad_enabled()))
        w = 1.0 if use_original_attn else 1.0 + routing_score[0, :, 1].float().mean().to(hidden_states.dtype)
        out = attn.to_q(hidden_states) * w
        if encoder_hidden_states is None:  # Wan self attention
            return out
        return out, attn.to_k(encoder_hidden_states) * w


class _CrossStub:
    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, rotary_emb=None):
        return attn.to_q(hidden_states)


def _spread_routers(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if type(m).__name__ == "Router":
            m.linear.weight.data = (torch.randn(m.linear.weight.shape, generator=g) * 0.5).to(m.linear.weight)
            m.linear.bias.data = (torch.randn(m.linear.bias.shape, generator=g) * 2.0).to(m.linear.bias)


def _stub_out(bound, log):
    bound.inner = _Stub(log, bound.layer)
    bound._accepted = set(inspect.signature(bound.inner.__call__).parameters)


def _hy(seed=0, differentiable=True, train_router=True):
    from vorta.patch.modeling_hunyuan import apply_vorta_transformer
    from vorta.patch.utils import prepare_hunyuan_self_attn_kwargs
    torch.manual_seed(seed)
    model = M.MiniHunyuanTransformer().to(BF)
    apply_vorta_transformer(model, train_router=train_router, router_dtype=BF,
                            attn_processor_kwargs=dict(differentiable=differentiable) if train_router else None)
    _spread_routers(model, seed + 1)
    log = []
    blocks = list(model.transformer_blocks) + list(model.single_transformer_blocks)
    for b in blocks:
        _stub_out(b.attn.processor, log)
    g = torch.Generator().manual_seed(seed + 2)
    mask = torch.zeros(1, 16)
    mask[:, :11] = 1
    inp = dict(hidden_states=torch.randn(1, 4, 4, 6, 8, generator=g).to(BF), timestep=torch.tensor([637.0]),
               encoder_hidden_states=torch.randn(1, 16, 24, generator=g).to(BF), encoder_attention_mask=mask,
               pooled_projections=torch.randn(1, 16, generator=g).to(BF))
    kw = prepare_hunyuan_self_attn_kwargs(dict(KW), torch.device("cpu"), None if train_router else 0.3)
    return model, blocks, inp, kw, log, model.time_text_embed.timestep_embedder


def _wan(seed=0):
    from vorta.patch.modeling_wan import apply_vorta_transformer
    from vorta.patch.utils import prepare_wan_self_attn_kwargs
    torch.manual_seed(seed)
    model = M.MiniWanTransformer().to(BF)
    apply_vorta_transformer(model, train_router=True, router_dtype=BF, attn_processor_kwargs=dict(differentiable=True))
    _spread_routers(model, seed + 1)
    log = []
    blocks = list(model.blocks)
    for b in blocks:
        assert b.attn2.processor.differentiable  # the training graph passes through the cross attention
        _stub_out(b.attn1.processor, log)
        b.attn2.processor = _CrossStub()
    g = torch.Generator().manual_seed(seed + 2)
    inp = dict(hidden_states=torch.randn(1, 4, 4, 6, 8, generator=g).to(BF), timestep=torch.tensor([412.0]),
               encoder_hidden_states=torch.randn(1, 20, 24, generator=g).to(BF))
    kw = prepare_wan_self_attn_kwargs(dict(KW), torch.device("cpu"))
    return model, blocks, inp, kw, log, model.condition_embedder.time_embedder


def _loss(model, sample, seed=5):
    from vorta.patch import routing_scores_of
    cot = torch.randn(sample.shape, generator=torch.Generator().manual_seed(seed))
    scores = routing_scores_of(model)
    return (sample.float() * cot).sum() + sum((s[..., 0].float() ** 2).mean() for s in scores)


def _checkpoint_blocks(blocks, use_reentrant=False):
    for b in blocks:
        b.forward = lambda *a, _f=b.forward, **k: checkpoint(_f, *a, use_reentrant=use_reentrant, **k)


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_graph_scores_are_forward_autograd_and_gradients_reach_every_router(family):
    from vorta.patch import routing_scores_of
    model, blocks, inp, kw, log, embedder = (_hy if family == "hunyuan" else _wan)()
    seen = []
    h = embedder.register_forward_hook(lambda m, a, o: seen.append(o))
    out = model(**inp, return_dict=False, self_attention_kwargs=kw, return_routing_scores=True)
    h.remove()
    assert len(out) == 5 and out[1] is None and out[2] is None and out[3] is None
    scores = routing_scores_of(model)
    assert scores.requires_grad and scores.shape == (len(blocks), 1, M.H, 3) and scores.dtype == BF
    assert len(log) == len(blocks)
    for layer, (block, call) in enumerate(zip(blocks, log)):
        want = block.router.forward_autograd(seen[0])
        assert torch.equal(scores[layer], want) and torch.equal(call["score"], want)
        assert call["score"].requires_grad and call["layer"] == layer and not call["teacher"]
        # the tuple's fifth element keeps the reference's meaning: detached CPU copies
        assert torch.equal(out[4][layer], want.detach()) and not out[4][layer].requires_grad
    _loss(model, out[0]).backward()
    for block in blocks:
        for p in (block.router.linear.weight, block.router.linear.bias):
            assert p.grad is not None and torch.isfinite(p.grad.float()).all() and p.grad.float().abs().sum() > 0
    # the timestep embedding is not detached on this path: a trainable embedder gets its gradient through the routers
    assert embedder.linear_2.weight.grad is not None and embedder.linear_2.weight.grad.float().abs().sum() > 0


# ------------------------------------------------------------------------------------------------------------------ (b)
def _count_route_plan(monkeypatch, L=4):
    from vorta_amd.patch import _engine as E
    calls = []

    def fake(x, w, b, heads, tau, num_experts):
        calls.append(tau)
        B = x.shape[0]
        return (torch.full((L, B, heads, num_experts), 1.0 / 3, dtype=x.dtype), torch.zeros((L, heads), dtype=torch.int32),
                torch.zeros((L, num_experts, heads), dtype=torch.int32), torch.zeros((L, num_experts), dtype=torch.int32))

    monkeypatch.setattr(E.ops, "route_plan", fake)
    return calls


def test_no_grad_and_frozen_routers_take_the_route_plan(monkeypatch):
    from vorta.patch import routing_scores_of
    calls = _count_route_plan(monkeypatch)
    model, blocks, inp, kw, log, _ = _hy(seed=3)
    with torch.no_grad():
        model(**inp, return_dict=False, self_attention_kwargs=kw)
    assert len(calls) == 1 and not routing_scores_of(model).requires_grad
    assert all(not c["score"].requires_grad for c in log)

    model, blocks, inp, kw, log, _ = _hy(seed=3)  # a fresh plan: its first call allocates through ops.route_plan
    model.requires_grad_(False)
    inp["hidden_states"].requires_grad_(True)
    out = model(**inp, return_dict=False, self_attention_kwargs=kw)
    assert len(calls) == 2 and out[0].requires_grad
    assert not routing_scores_of(model).requires_grad and all(not c["score"].requires_grad for c in log)

    model, blocks, inp, kw, log, _ = _hy(seed=3)  # trainable routers in grad mode: no route plan at all
    out = model(**inp, return_dict=False, self_attention_kwargs=kw)  # (held: the scores' graph lives with the output)
    assert len(calls) == 2 and routing_scores_of(model).requires_grad
    del out

    model, blocks, inp, kw, log, _ = _hy(seed=3, train_router=False)  # the inference patch in grad mode: unchanged
    model(**inp, return_dict=False, self_attention_kwargs=kw)
    assert len(calls) == 3 and calls[-1] == 0.3 and not routing_scores_of(model).requires_grad


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_recomputed_blocks_get_their_own_forwards_state_and_it_is_released(family, monkeypatch):
    from vorta.patch import original_attention, routing_scores_of
    model, blocks, inp, kw, log, _ = (_hy if family == "hunyuan" else _wan)(seed=7)
    _count_route_plan(monkeypatch, L=len(blocks))  # (the no_grad forward in between takes the route plan)
    _checkpoint_blocks(blocks)
    out = model(**inp, return_dict=False, self_attention_kwargs=kw)
    student = list(log)
    assert len(student) == len(blocks) and all(c["grad_mode"] and not c["teacher"] for c in student)
    with original_attention(model), torch.no_grad():
        teacher = model(**inp, return_dict=False)[0]  # no keyword set needed, no route plan computed
    assert len(log) == 2 * len(blocks) and all(c["teacher"] and c["score"] is None for c in log[len(blocks):])
    assert teacher.shape == out[0].shape and not torch.equal(teacher, out[0])
    with torch.no_grad():  # another student forward in between, with another keyword set
        other_kw = dict(kw)
        model(**inp, return_dict=False, self_attention_kwargs=other_kw)
    assert routing_scores_of(model).requires_grad is False
    del log[:]
    loss = (out[0].float() * torch.randn(out[0].shape, generator=torch.Generator().manual_seed(5))).sum()
    loss.backward()
    # non-reentrant checkpointing recomputes every block once, in whatever order the backward needs them
    assert sorted(c["layer"] for c in log) == list(range(len(blocks)))
    for c in log:
        first = student[c["layer"]]
        assert c["teacher"] is False
        assert c["score"] is first["score"] and c["group"] is first["group"] and c["descriptor"] is first["descriptor"]
    for block in blocks:
        assert block.router.linear.weight.grad is not None and block.router.linear.bias.grad is not None
    alive = [weakref.ref(student[0]["score"]), weakref.ref(student[-1]["score"])]
    del loss, out, student, first, c
    del log[:]
    gc.collect()
    assert all(r() is None for r in alive), "the forward's scores outlive everything that could run its backward"
    from vorta_amd.patch import _engine as E
    ctx = E.context_of(model)  # nothing of the three forwards is left but the latest student's detached scores
    assert ctx.current is None and not ctx.records and ctx.student() is None and not routing_scores_of(model).requires_grad


def test_scores_are_released_without_checkpointing_too():
    from vorta.patch import routing_scores_of
    model, blocks, inp, kw, log, _ = _hy(seed=9)
    out = model(**inp, return_dict=False, self_attention_kwargs=kw)
    scores = routing_scores_of(model)
    assert scores.requires_grad
    alive = weakref.ref(scores)
    loss = _loss(model, out[0])
    del scores, out
    del log[:]
    gc.collect()
    assert alive() is not None and routing_scores_of(model).requires_grad  # the loss still holds the graph
    del loss
    gc.collect()
    assert alive() is None
    assert not routing_scores_of(model).requires_grad  # what is left of that forward: the values


def test_reentrant_checkpoint_is_refused_with_a_clear_error():
    model, blocks, inp, kw, log, _ = _hy(seed=11)
    _checkpoint_blocks(blocks, use_reentrant=True)
    inp["hidden_states"].requires_grad_(True)
    out = model(**inp, return_dict=False, self_attention_kwargs=kw)
    with pytest.raises(RuntimeError, match="use_reentrant=False"):
        out[0].float().sum().backward()


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_original_attention_restores_the_flag_after_an_exception():
    from vorta.patch import original_attention
    from vorta_amd.patch import _engine as E
    model, blocks, inp, kw, log, _ = _hy(seed=13)
    ctx = E.context_of(model)
    with pytest.raises(KeyError):
        with original_attention(model):
            assert ctx.teacher
            with original_attention(model):  # nests
                pass
            assert ctx.teacher
            raise KeyError("inside")
    assert ctx.teacher is False
    model(**inp, return_dict=False, self_attention_kwargs=kw)
    assert len(log) == len(blocks) and not any(c["teacher"] for c in log)
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        with original_attention(M.MiniHunyuanTransformer()):
            pass


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_return_losses_stays_refused_on_a_trainable_model():
    model, blocks, inp, kw, log, _ = _hy(seed=15)
    with pytest.raises(NotImplementedError):
        model(**inp, self_attention_kwargs=kw, return_losses=True)
    with pytest.raises(NotImplementedError):
        model(**inp, self_attention_kwargs=kw, reture_hidden_layer_distill_loss=True)
    out = model(**inp, self_attention_kwargs=kw)  # and the refusal leaves nothing behind
    assert out.sample.requires_grad and len(log) == len(blocks)
