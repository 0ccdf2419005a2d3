"""GPU: router training through the patched transformers -- `apply_vorta_transformer(model, train_router=True,
attn_processor_kwargs={"differentiable": True})` on the mini models of tests/_mini_diffusers.py at the geometry of
tests/test_hip_patch.py (latent (4, 6, 8) = 192 tokens, tile (2, 3, 4), window (3, 3, 3), group (2, 3, 2), text 16 with 11
valid: coreset duplicates, sliding groups with tails, padded text and a partial 256-row block).

The loss is a fixed random cotangent on the output plus the reference's regulariser on `routing_scores_of(model)`.  Every
test runs the `deterministic` attention backward and restores the previous selection.

Accuracy (test 3): per router weight and bias, the relative Frobenius error against float64 autograd of the restated whole
model (tests/_patch_training_restate.py, on the CPU) is at most 2 x that of torch's own 16-bit autograd of the same
restatement -- the project's standing bound (tests/test_hip_attention_bwd.py).  VORTA_PATCH_TRAINING_ACCURACY_OUT names a
file that receives the ratios (profiles/patch_training_accuracy.txt is such a file)."""
import os

import numpy as np
import pytest
import torch
from torch.utils.checkpoint import checkpoint

import _mini_diffusers as M
import _patch_training_restate as R
from _norm_rope_restate import rel_err
from _util import dev

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, GROUP = (4, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)
T, TE = 16, 11
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = [("hunyuan", "bf16"), ("wan", "bf16"), ("hunyuan", "fp16")]
IDS = ["-".join(c) for c in CASES]
RATIOS = {}
_RUNS = {}


@pytest.fixture(autouse=True)
def _deterministic_backward():
    from vorta_amd import routed, set_attention_backward
    previous = routed._attention_backward
    set_attention_backward("deterministic")
    yield
    routed._attention_backward = previous


def _spread_routers(model, seed):  # tests/test_hip_patch.py: wide logits, layers that disagree
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if type(m).__name__ == "Router":
            m.linear.weight.data = (torch.randn(m.linear.weight.shape, generator=g) * 0.5).to(m.linear.weight)
            m.linear.bias.data = (torch.randn(m.linear.bias.shape, generator=g) * 2.0).to(m.linear.bias)


def _geometry():
    return dict(latent_shape=LATENT, window_size=WINDOW, tile_size=TILE, lowres_window_size=GROUP, lowres_reduction_rate=0.5)


def _model(family, dtype, seed=0, dense=False):
    """the mini model of `family` with the weights of `seed`: routed for training, or (dense) the native-attention patch"""
    import vorta.patch.modeling_hunyuan as mh
    import vorta.patch.modeling_wan as mw
    mod = mh if family == "hunyuan" else mw
    torch.manual_seed(seed)
    model = (M.MiniHunyuanTransformer if family == "hunyuan" else M.MiniWanTransformer)().to(dev()).to(dtype)
    if dense:
        return mod.apply_sp_flashattn_transformer(model)
    mod.apply_vorta_transformer(model, train_router=True, router_dtype=dtype, attn_processor_kwargs={"differentiable": True})
    _spread_routers(model, seed + 1)
    return model


def _kwargs(family):
    from vorta.patch.utils import prepare_hunyuan_self_attn_kwargs, prepare_wan_self_attn_kwargs
    prepare = prepare_hunyuan_self_attn_kwargs if family == "hunyuan" else prepare_wan_self_attn_kwargs
    return prepare(_geometry(), dev())


def _inputs(family, dtype, seed=1):
    g = torch.Generator(device=dev()).manual_seed(seed)
    hidden = torch.randn((1, 4) + LATENT, device=dev(), generator=g).to(dtype)
    if family == "wan":
        return dict(hidden_states=hidden, timestep=torch.tensor([412.0], device=dev()),
                    encoder_hidden_states=torch.randn((1, 20, 24), device=dev(), generator=g).to(dtype))
    mask = torch.zeros((1, T), device=dev())
    mask[:, :TE] = 1
    return dict(hidden_states=hidden, timestep=torch.tensor([637.0], device=dev()),
                encoder_hidden_states=torch.randn((1, T, 24), device=dev(), generator=g).to(dtype),
                encoder_attention_mask=mask, pooled_projections=torch.randn((1, 16), device=dev(), generator=g).to(dtype),
                guidance=torch.tensor([6000.0], device=dev()).to(dtype))


def _cotangent(dtype):
    return torch.randn((1, 4) + LATENT, generator=torch.Generator().manual_seed(17)).to(dtype).to(dev())


def _student(model, family, inp, dtype):
    """one training forward + its loss; the hidden states are a fresh leaf"""
    from vorta.patch import routing_scores_of
    inp = dict(inp, hidden_states=inp["hidden_states"].detach().clone().requires_grad_(True))
    out = model(**inp, return_dict=False, self_attention_kwargs=_kwargs(family), return_routing_scores=True)
    scores = routing_scores_of(model)
    return inp, out, scores, R.training_loss(out[0], scores, _cotangent(dtype), torch.float32)


def _leaves(model, inp):
    return list(R.router_parameters(model).values()) + [inp["hidden_states"]]


def _run(family, dtype_name):
    """the un-checkpointed training step of one case, once per session: model, inputs, outputs, recorded launches, gradients"""
    key = (family, dtype_name)
    if key not in _RUNS:
        dtype = DTYPES[dtype_name]
        model = _model(family, dtype)
        with R.RecordLaunches() as rec:
            inp, out, scores, loss = _student(model, family, _inputs(family, dtype), dtype)
        loss.backward()
        torch.cuda.synchronize()
        names = list(R.router_parameters(model)) + ["hidden_states"]
        _RUNS[key] = dict(model=model, dtype=dtype, inp=inp, sample=out[0].detach(), tuple_scores=out[4], scores=scores.detach(),
                          graph=scores.requires_grad, recorded=list(rec.calls),
                          grads={n: (None if t.grad is None else t.grad.clone()) for n, t in zip(names, _leaves(model, inp))})
    return _RUNS[key]


# -------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_loss_backward_reaches_every_router(family):
    run = _run(family, "bf16")
    assert run["graph"], "routing_scores_of must hand out the graph-carrying scores of a training forward"
    n_layers = len(R.blocks_of(run["model"]))
    assert len(run["recorded"]) == n_layers and len(run["grads"]) == 2 * n_layers + 1
    for name, g in run["grads"].items():
        assert g is not None, f"{family}: no gradient for {name}"
        assert torch.isfinite(g.float()).all() and g.float().abs().sum() > 0, f"{family}: {name}"


# -------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("family,dtype_name", CASES, ids=IDS)
def test_training_forward_gives_the_no_grad_bits(family, dtype_name):
    from vorta.patch import routing_scores_of
    run = _run(family, dtype_name)
    model = run["model"]
    with torch.no_grad():
        plain = model(**run["inp"], return_dict=False, self_attention_kwargs=_kwargs(family), return_routing_scores=True)
    detached = routing_scores_of(model)
    assert not detached.requires_grad
    n = int((detached != run["scores"]).sum())
    print(f"{family} {dtype_name}: scores of Router.forward_autograd that differ from the route plan's: {n} of {detached.numel()}")
    assert torch.equal(detached, run["scores"]), "the training path's scores must be the route plan's bits"
    assert torch.equal(plain[0], run["sample"])
    for layer in range(len(R.blocks_of(model))):
        assert torch.equal(run["tuple_scores"][layer], run["scores"][layer].cpu())
        assert torch.equal(plain[4][layer], run["tuple_scores"][layer]) and not run["tuple_scores"][layer].requires_grad


# -------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("family,dtype_name", CASES, ids=IDS)
def test_router_gradients_against_float64(family, dtype_name):
    run = _run(family, dtype_name)
    cot = _cotangent(run["dtype"])
    ref, o64 = R.reference_gradients(run["model"], run["inp"], run["recorded"], cot, torch.float64, "cpu")
    t16, _ = R.reference_gradients(run["model"], run["inp"], run["recorded"], cot, run["dtype"], dev())
    e_fwd = rel_err(run["sample"].cpu(), o64)
    print(f"{family} {dtype_name}: forward against the float64 restatement {e_fwd:.3e}")
    pairs = {}
    for name in ref:
        e_hip, e_t = rel_err(run["grads"][name].cpu(), ref[name]), rel_err(t16[name].cpu(), ref[name])
        print(f"{family} {dtype_name} {name}: e_hip {e_hip:.3e} e_torch {e_t:.3e} ratio {e_hip / max(e_t, 1e-300):.3f}")
        RATIOS[f"{family} {dtype_name} {name}"] = (e_hip, e_t)
        pairs[name] = (e_hip, e_t)
    # one processor call lies within 1.5e-2 of its restatement (tests/test_hip_processors_grad.py); the layers' errors add
    assert e_fwd < 1.5e-2 * len(run["recorded"]), "the restatement does not state this model's forward"
    for name, (e_hip, e_t) in pairs.items():
        assert e_hip <= 2.0 * e_t, f"{family} {dtype_name} {name}: e_hip {e_hip:.3e} > 2 x e_torch {e_t:.3e}"


# -------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_checkpointed_blocks_give_the_unchecked_bits_with_a_teacher_pass_in_between(family):
    from vorta.patch import original_attention
    run = _run(family, "bf16")
    model, dtype = run["model"], run["dtype"]
    blocks = R.blocks_of(model)
    for b in blocks:
        b.forward = lambda *a, _f=b.forward, **k: checkpoint(_f, *a, use_reentrant=False, **k)
    try:
        inp, out, scores, loss = _student(model, family, run["inp"], dtype)
        assert torch.equal(out[0], run["sample"])
        with original_attention(model), torch.no_grad():
            teacher = model(**run["inp"], return_dict=False)[0]
        assert not torch.equal(teacher, run["sample"])
        names = list(run["grads"])
        passes = [torch.autograd.grad(loss, _leaves(model, inp), retain_graph=True) for _ in range(5)]
        torch.cuda.synchronize()
    finally:
        for b in blocks:
            del b.forward
    for name, g in zip(names, passes[0]):
        assert torch.equal(g, run["grads"][name]), f"{family}: {name} differs from the un-checkpointed run: the recompute " \
                                                     "saw other scores, keywords or tables"
    for i, p in enumerate(passes[1:]):
        for name, g, first in zip(names, p, passes[0]):
            assert torch.equal(g, first), f"{family}: {name} of backward pass {i + 2} differs from the first"


# -------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_teacher_pass_is_the_native_attention_model(family):
    from vorta.patch import original_attention
    run = _run(family, "bf16")
    model, dtype = run["model"], run["dtype"]
    with original_attention(model), torch.no_grad():
        teacher = model(**run["inp"], return_dict=False, return_routing_scores=True)
    assert len(teacher) == 5 and teacher[4] == []  # the routed protocol, and no route plan
    dense = _model(family, dtype, dense=True)  # same seed: the same weights
    with torch.no_grad():
        want = dense(**run["inp"], return_dict=False)[0]
    assert torch.equal(teacher[0], want)
    inp, out, scores, loss = _student(model, family, run["inp"], dtype)  # a student forward after it is unaffected
    assert scores.requires_grad and torch.equal(out[0], run["sample"]) and torch.equal(scores.detach(), run["scores"])


# --------------------------------------------------------------------------------------------------------------- record
def test_accuracy_summary_written():
    """the ratios of this module's cases (runs after them)"""
    if not RATIOS:
        return
    lines = [f"  {name}: {e:.3e} / {e_t:.3e} = {e / max(e_t, 1e-300):.3f}" for name, (e, e_t) in RATIOS.items()]
    r = [e / max(e_t, 1e-300) for e, e_t in RATIOS.values()]
    lines.append(f"all {len(r)} gradients: max {max(r):.3f} median {float(np.median(r)):.3f}")
    print("\n".join(lines))
    path = os.environ.get("VORTA_PATCH_TRAINING_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("tests/test_hip_patch_training.py: router gradients of the patched mini transformers, deterministic backward\n"
                    "error against float64 autograd of the restated model / error of torch's 16-bit autograd of it (bound: 2)\n"
                    + "\n".join(lines) + "\n")
