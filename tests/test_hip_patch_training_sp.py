"""GPU: router training through the patched transformers UNDER SEQUENCE PARALLELISM -- `apply_vorta_transformer(model,
train_router=True, attn_processor_kwargs={"differentiable": True})` with `SP_STATE` enabled and grad mode on, frame-sharded
and inside `token_sharded(model)`, `all_reduce_router_grads(model)` afterwards, and the Wan cross attention that such a
graph passes through.  gloo ranks share the one GPU (the spawn pattern of tests/test_hip_sp_soft_mixture.py: at most 4
ranks, one time limit per spawn, a failed or late worker fails the test); the workers are tests/_patch_training_sp.py.

Models and geometry: tests/test_hip_patch_training.py -- latent (4, 6, 8) = 192 tokens, 96 per rank of two and 48 per rank
of four: coreset duplicates, sliding groups with tails, padded text (16 rows, 11 valid), partial 256-row blocks, T <= S/P.
Truth: float64 autograd of the restated whole model (tests/_patch_training_restate.py) fed the launches the ranks recorded.
Bounds, none of them new: per gradient, the relative Frobenius error is at most 2 x that of torch's own 16-bit autograd of
the same restatement; for a forward, the sequence-parallel error against float64 is at most 2 x the single-process error.
Every worker runs the `deterministic` attention backward and restores the previous choice.
VORTA_PATCH_TRAINING_SP_ACCURACY_OUT names a file that receives the ratios (profiles/patch_training_sp_accuracy.txt)."""
import os
import re

import numpy as np
import pytest

import _patch_training_sp as W
import test_hip_sp_soft_mixture as SM

pytestmark = pytest.mark.gpu

FIGURES = []  # (kind, case, name, e, e_yardstick) of every bound checked in this module
_SPAWNS = {}
FRAME_CASES = [("hunyuan", "bf16"), ("wan", "bf16"), ("hunyuan", "fp16")]
TOKEN_CASES = [("hunyuan", 2), ("hunyuan", 4), ("wan", 2), ("wan", 4)]


@pytest.fixture(autouse=True)
def _deterministic_backward():
    from vorta_amd import routed, set_attention_backward
    previous = routed._attention_backward
    set_attention_backward("deterministic")
    yield
    routed._attention_backward = previous


def _exit_codes(error):
    """the list of exit codes SM._run's assertion carries in front of its message"""
    m = re.match(r"\s*\[([^\]]*)\]", str(error))
    return [int(x) for x in re.findall(r"-?\d+", m.group(1))] if m else [None]


def _spawn(target, world, args):
    """one spawn per case and session, shared by the tests that read it; a spawn that failed is not started again"""
    key = (target.__name__, world) + tuple(args)
    if key not in _SPAWNS:
        # a worker that died of a signal or ran out of time (SM._run reports the exit codes; 1 is a Python exception):
        # nothing more is started on the GPU by this module
        stopped = [k for k, v in _SPAWNS.items() if isinstance(v, AssertionError) and set(_exit_codes(v)) - {0, 1}]
        assert not stopped, f"not started: the ranks of {stopped[0]} ended with {_exit_codes(_SPAWNS[stopped[0]])}"
        try:
            _SPAWNS[key] = SM._run(target, world, tuple(args), limit=200)
        except BaseException as e:  # noqa: BLE001
            _SPAWNS[key] = e
    if isinstance(_SPAWNS[key], BaseException):
        raise AssertionError(f"the ranks of {key} failed: {_SPAWNS[key]!r}")
    return _SPAWNS[key]


def _frame(family, dtype):
    return _spawn(W.model_worker, 2, (family, dtype, "frame", "even", ("fidelity",) if dtype == "bf16" else ()))


def _token(family, world):
    return _spawn(W.model_worker, world, (family, "bf16", "token", "even", ("checkpoint", "fidelity") if world == 2 else ()))


def _check(kind, case, pairs):
    """every (error, yardstick error) pair: printed and kept first, then the bound e <= 2 x yardstick"""
    for name, (e, e_y) in pairs.items():
        print(f"{kind} {case} {name}: e {e:.3e} yardstick {e_y:.3e} ratio {e / max(e_y, 1e-300):.3f}")
        FIGURES.append((kind, case, name, e, e_y))
    for name, (e, e_y) in pairs.items():
        assert e <= 2.0 * e_y, f"{kind} {case} {name}: e {e:.3e} > 2 x {e_y:.3e}"


def _check_model(kind, case, res):
    assert not res["missing"], f"{case}: no gradient for {res['missing']}"
    # every router weight and bias of every layer, the latent and the text
    assert len(res["bwd"]) == 2 * res["layers"] + 2 and set(res["bwd"]) == set(res["names"]), sorted(res["bwd"])
    # the text gradient: whole on every Hunyuan rank (its text stream carries whole cotangents between the layers), a share
    # per Wan rank; the other reading of the same tensors, for the record
    print(f"{kind} {case} encoder_hidden_states, read the other way: e {res['text_grad_other_reading']:.3e}")
    if case.startswith("hunyuan"):
        assert res["text_grad_equal_on_every_rank"]
    assert res["same_as_no_grad"], "the training forward must give the bits of the same call under torch.no_grad()"
    assert res["ranks_agree_after_reduce"]
    _check(kind + ", forward (SP vs one process, against float64)", case, {"sample": res["fwd"]})
    _check(kind + ", backward (SP vs torch 16-bit autograd, against float64)", case, res["bwd"])


# -------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("branch", ["text", "image"])
def test_wan_cross_attention_trains_locally_under_sequence_parallel(branch):
    """WanAttnProcessor2_0(differentiable=True) with encoder_hidden_states on two ranks' query shards: text keys only, and
    257 image tokens through add_k_proj / add_v_proj / norm_added_k in front of them"""
    res = _spawn(W.wan_cross_worker, 2, ("bf16",))[branch]
    assert res["graph"] == [True, True], "the call must build an autograd graph"
    assert res["bits"] == [True, True], "grad mode must give the bits of the no_grad call"
    assert res["calls"] == [{}, {}], f"cross attention has replicated keys and needs no collective: {res['calls']}"
    assert not res["missing"], res["missing"]
    assert len(res["bwd"]) == (11 if branch == "image" else 8)
    print(f"Wan cross attention {branch}: forward against float64 {res['fwd'][0]:.3e} (torch 16-bit {res['fwd'][1]:.3e})")
    assert res["fwd"][0] < 1.5e-2, "the restatement does not state this forward (tests/test_hip_processors_grad.py)"
    _check("Wan cross attention, backward (hidden shards concatenated; enc and parameters summed over the ranks)", branch,
           res["bwd"])


# -------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("family,dtype", FRAME_CASES, ids=["-".join(c) for c in FRAME_CASES])
def test_whole_model_trains_frame_sharded(family, dtype):
    """every rank passes its latent frames; loss = sum(out_shard * cot_shard) + reg(scores) / P; router gradients after
    all_reduce_router_grads(op="sum") and the concatenated latent gradient against float64"""
    res = _frame(family, dtype)["res"]
    assert res["out_shape"] == (1, 4, 2, 6, 8)
    assert res["zeros_ok"], "before the reduce, score gradients outside a rank's heads must be exactly zero"
    _check_model("frame shard, 2 ranks", f"{family} {dtype}", res)


# -------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("family,world", TOKEN_CASES, ids=[f"{f}-w{w}" for f, w in TOKEN_CASES])
def test_whole_model_trains_token_sharded(family, world):
    """whole latents on every rank inside token_sharded(model), the same loss on the whole output, reg / P; router
    gradients after the sum and the latent gradients summed over the ranks against float64"""
    res = _token(family, world)["res"]
    assert res["out_shape"] == (1, 4, 4, 6, 8)
    assert res["plain_equal_on_every_rank"], "every rank must hold the same gathered output"
    assert res["zeros_ok"]
    _check_model(f"token shard, {world} ranks", f"{family} bf16", res)


# -------------------------------------------------------------------------------------------------------------------- 4
def test_a_latent_whose_frames_the_ranks_do_not_divide_trains_token_sharded():
    g, P = W.GEOMS["odd"], 2
    S = int(np.prod(g["latent"]))
    # the choice, checked on the host first: tokens divide, frames do not, the text fits a shard, the tile divides the latent
    assert g["latent"][0] % P != 0 and S % P == 0 and W.T_TEXT <= S // P
    assert all(l % t == 0 for l, t in zip(g["latent"], g["tile"])) and all(l % w == 0 for l, w in zip(g["latent"], g["group"]))
    res = _spawn(W.model_worker, P, ("hunyuan", "bf16", "token", "odd", ("refuse_frames",)))["res"]
    assert "frame" in res["refusal"] and f" {g['latent'][0]} " in res["refusal"], res["refusal"]
    assert res["out_shape"] == (1, 4) + g["latent"]
    assert res["plain_equal_on_every_rank"] and res["zeros_ok"]
    _check_model("token shard, 2 ranks, 3 latent frames", "hunyuan bf16", res)


# -------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_checkpointed_blocks_with_a_teacher_pass_in_between_give_the_unchecked_bits(family):
    """token-sharded, 2 ranks, every block under a non-reentrant checkpoint, an original_attention(model) forward under
    no_grad between forward and backward: PER RANK the gradients before the reduce are the un-checkpointed run's bits, and
    two backward passes of one forward agree (sums across ranks are outside that claim)"""
    ret = _token(family, 2)
    for rank in range(2):
        ck = ret[f"rank {rank}"]["checkpoint"]
        assert ck["out_equal"] and ck["teacher_differs"] and ck["teacher_shape"] == (1, 4, 4, 6, 8), (rank, ck)
        assert not ck["differ_from_unchecked"], (rank, ck["differ_from_unchecked"])
        assert not ck["differ_between_passes"], (rank, ck["differ_between_passes"])


# -------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_expert_fidelity_inside_token_sharded(family):
    """fidelity_of(model) after a forward under expert_fidelity inside token_sharded: all H heads of every layer on every
    rank, and the values of the same forward on frame shards -- the blocks see the same tokens either way"""
    token, frame = _token(family, 2), _frame(family, "bf16")
    L, H = token["res"]["layers"], 4
    first = token["rank 0"]["fidelity"]
    for rank in range(2):
        fid = token[f"rank {rank}"]["fidelity"]
        assert fid["shapes"] == [(L, H), (L, H), (L, H, 3), (L, H, 3)], fid["shapes"]
        assert fid["out_same"], "measuring must not change the output"
        for n in W.FID_FIELDS:
            assert np.isfinite(fid["values"][n]).all() and (fid["values"][n][..., :2] > 0).all(), n
            assert np.array_equal(fid["values"][n], first["values"][n]), f"{n}: the ranks hold different statistics"
            other = frame[f"rank {rank}"]["fidelity"]["values"][n]
            print(f"{family} rank {rank} {n}: largest |token shard - frame shard| {np.abs(fid['values'][n] - other).max():.3e}")
            assert np.array_equal(fid["values"][n], other), f"{n}: token-sharded and frame-sharded forwards measured differently"


# --------------------------------------------------------------------------------------------------------------- record
def test_accuracy_summary_written():
    """the figures of this module's cases (runs after them)"""
    if not FIGURES:
        return
    lines = []
    for kind in dict.fromkeys(f[0] for f in FIGURES):
        lines.append(kind + ": error / yardstick error (bound: 2)")
        for _, case, name, e, e_y in (f for f in FIGURES if f[0] == kind):
            lines.append(f"  {case} {name}: {e:.3e} / {e_y:.3e} = {e / max(e_y, 1e-300):.3f}")
    r = [e / max(e_y, 1e-300) for _, _, _, e, e_y in FIGURES]
    lines.append(f"all {len(r)} figures: max {max(r):.3f} median {float(np.median(r)):.3f}")
    print("\n".join(lines))
    path = os.environ.get("VORTA_PATCH_TRAINING_SP_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("tests/test_hip_patch_training_sp.py: gloo ranks sharing one MI355X (host-staged transport), deterministic "
                    "backward\n" + "\n".join(lines) + "\n")
