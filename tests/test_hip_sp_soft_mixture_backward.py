"""GPU: the key-major and the deterministic attention backward under sequence parallelism --
`sp_soft_mixture_attention_autograd(backward=...)`, `set_attention_backward` / VORTA_ATTENTION_BACKWARD and the
`differentiable=True` Train processors -- on gloo ranks that share the one GPU, plus one case on a real RCCL group of one rank.

Shapes, cases and float64 references: tests/_sp_soft_mixture.py (latent (12, 6, 8), S = 576: S/P = 288 and 144 are no
multiples of the 128 query rows of a workgroup, and 576 keys leave a partial 256-key block; Hunyuan 8 text rows with 5 valid).
Workers: tests/_sp_backward_workers.py.  Spawning: `_run` of tests/test_hip_sp_soft_mixture.py.

Bound (not new): per gradient, the error against float64 autograd of the restated launches is at most 2 x that of torch's own
16-bit autograd on the same restatement (`test_hip_sp_soft_mixture._check`).
One run per case is shared by the gradient, repeat and precondition tests (`_case`).  VORTA_SP_BACKWARD_ACCURACY_OUT names a
file that receives the figures (profiles/sp_soft_mixture_backward_accuracy.txt is such a file)."""
import json
import os
import subprocess
import sys

import pytest

import _sp_backward_workers as W
import _sp_soft_mixture as C
from test_hip_sp_soft_mixture import _free_port, _run

pytestmark = pytest.mark.gpu
ROOT = C.ROOT
FIGURES = []  # (kind, case, name, e, e_yardstick) of every bound checked in this module
REPEATS = {}  # case -> (backward passes, every rank's dq, dk, dv, dscores equal across them)
BITS = {}     # case -> {dq, dk, dv: assembled bits equal to the single-process operator's under the same algorithm}
SHAPES = {"w2h4": (2, 4), "w4h4": (4, 4), "w2h3_uneven": (2, 3)}
_CASES = {}


def _name(shape, model, dtype, algorithm):
    world, H = SHAPES[shape]
    return f"{algorithm} {model} world {world} H {H} {dtype}"


def _case(shape, model, dtype, algorithm):
    """the ranks' run of one case, once per session: five backward passes where the repeat test looks (deterministic, two
    ranks, bf16), one elsewhere"""
    key = (shape, model, dtype, algorithm)
    if key not in _CASES:
        world, H = SHAPES[shape]
        repeats = 5 if (algorithm == "deterministic" and world == 2 and dtype == "bf16") else 1
        _CASES[key] = _run(W.gradient_worker, world, (model, H, dtype, algorithm, repeats))["res"]
    return _CASES[key]


def _check(kind, case, pairs):
    """every (error, yardstick error) pair: printed and kept first, then the bound e <= 2 x yardstick"""
    for name, (e, e_y) in pairs.items():
        print(f"{kind} {case} {name}: e {e:.3e} yardstick {e_y:.3e} ratio {e / max(e_y, 1e-300):.3f}")
        FIGURES.append((kind, case, name, e, e_y))
    for name, (e, e_y) in pairs.items():
        assert e <= 2.0 * e_y, f"{kind} {case} {name}: e {e:.3e} > 2 x {e_y:.3e}"


GRADIENT_CASES = ([("deterministic", s, m, "bf16") for s in SHAPES for m in ("hunyuan", "wan")]
                  + [("deterministic", "w2h4", m, "fp16") for m in ("hunyuan", "wan")]
                  + [("key_major", "w2h4", m, "bf16") for m in ("hunyuan", "wan")])


# ------------------------------------------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_dispatch_follows_keyword_switch_and_environment(model):
    """2: which entry points of vorta_amd.ops the backward of the operator calls on two ranks, per selection route; the
    choice is the one in force when the forward ran"""
    ret = _run(W.dispatch_worker, 2, (model,))
    want = {"nothing set": "query_major",
            "keyword deterministic": "deterministic",
            "keyword key_major": "key_major",
            "switch deterministic": "deterministic",
            "switch key_major": "key_major",
            "environment deterministic": "deterministic",
            "environment key_major": "key_major",
            "keyword deterministic over switch key_major": "deterministic",
            "switch over environment": "query_major",
            "forward deterministic, then switched to query_major": "deterministic",
            "forward with nothing set, then switched to deterministic": "query_major"}
    for rank in range(2):
        got = ret[rank]["scenarios"]
        assert set(got) == set(want)
        for name, algorithm in want.items():
            n = got[name]["n_launches"]
            assert n == (4 if model == "hunyuan" else 3)  # full, coreset, sliding (+ the sliding expert's text queries)
            assert got[name]["calls"] == W.expected_calls(algorithm, n), (rank, name, got[name])
        assert ret[rank]["keyword_equals_switch"], "deterministic by keyword and by switch must give the same bits"


def test_train_processors_follow_the_switch_under_sequence_parallel():
    """2: `differentiable=True` Train processors on two ranks run the algorithm of the process-wide switch"""
    ret = _run(W.processor_worker, 2, ())
    for rank in range(2):
        for which, n in (("wan", 3), ("hunyuan_single", 4)):
            for switch, algorithm in (("nothing set", "query_major"), ("deterministic", "deterministic"), ("key_major", "key_major")):
                got = ret[rank][f"{which} {switch}"]
                assert got["n_launches"] == n and got["finite"], (rank, which, switch, got)
                assert got["calls"] == W.expected_calls(algorithm, n), (rank, which, switch, got)


# ----------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("algorithm,shape,model,dtype", GRADIENT_CASES, ids=["-".join(c) for c in GRADIENT_CASES])
def test_gradients_against_float64(algorithm, shape, model, dtype):
    """3: the assembled gradients (video shards concatenated, text rows and score gradients summed over the ranks) against
    float64 autograd of the restated launches; exact zeros outside a rank's heads; one forward whatever the algorithm"""
    res = _case(shape, model, dtype, algorithm)
    world, H = SHAPES[shape]
    case = _name(shape, model, dtype, algorithm)
    assert res["counts"] == ([2, 1] if H == 3 else [H // world] * world)
    assert res["forward_same"], "the forward's bits must not depend on the backward's algorithm"
    assert res["restated_forward"] < 1.5e-2  # the restatement states this forward (tests/test_hip_sp_soft_mixture.py)
    for r in res["per_rank"]:
        assert r["calls"] == W.expected_calls(algorithm, r["n_launches"] * res["repeats"]), r
    _check("backward (kernels vs torch 16-bit autograd)", case, res["bwd"])
    assert res["zeros_ok"], "text rows / score gradients outside a rank's heads must be exactly zero"


# ------------------------------------------------------------------------------------------------------- same bits again
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("shape", ["w2h4", "w2h3_uneven"])
def test_deterministic_repeats_bit_for_bit(shape, model):
    """4: five backward passes of one forward per rank, each into freshly zeroed accumulators: every rank's dq, dk, dv and
    dscores are equal bit for bit.  Beside it, not asserted: whether the assembled gradients equal the single-process
    deterministic operator's bits."""
    res = _case(shape, model, "bf16", "deterministic")
    case = _name(shape, model, "bf16", "deterministic")
    assert res["repeats"] == 5
    same = [r["same_passes"] for r in res["per_rank"]]
    REPEATS[case] = (res["repeats"], all(all(s.values()) for s in same))
    BITS[case] = res["bits_equal_single_process"]
    print(f"{case}: equal across {res['repeats']} passes per rank: {same}; "
          f"assembled bits equal to the single-process operator's: {res['bits_equal_single_process']}")
    for rank, s in enumerate(same):
        for name, ok in s.items():
            assert ok, f"{case}: {name} of rank {rank} differs between two backward passes"


# -------------------------------------------------------------------------------------------------- the layout's promise
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_receive_layout_keeps_one_writer_per_row(shape, model):
    """5: from the launches every rank recorded -- distinct rows per key list, distinct heads per head list, and
    head * stride_h + row * stride_s one-to-one over the overlapping head views of the float32 accumulators (dq over a launch's
    (slot, query row) pairs, dk / dv over the (slot, key row) pairs of one key list), the text segment included"""
    res = _case(shape, model, "bf16", "deterministic")
    for rank, r in enumerate(res["per_rank"]):
        pre = r["pre"]
        print(f"{_name(shape, model, 'bf16', 'deterministic')} rank {rank}: {pre}")
        assert pre["launches"] == (4 if model == "hunyuan" else 3) and pre["key_lists"] > pre["launches"]  # (the sliding lists)
        assert pre["rows_distinct"] and pre["heads_distinct"], (rank, pre)
        assert pre["dq_one_to_one"] and pre["dkv_one_to_one"] and pre["inside"], (rank, pre)
        assert pre["text_rows_seen"] == (model == "hunyuan")


# ------------------------------------------------------------------------------------------------------------------ RCCL
def test_rccl_group_of_one_rank_deterministic():
    """6: forward + deterministic backward with the collectives forced through a real RCCL group of one rank (a fresh child)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0",
               VORTA_SP_FORCE_COLLECTIVES="1")
    env.pop("VORTA_ATTENTION_BACKWARD", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rccl_single_rank_sp_backward.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines and r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.loads(lines[-1])
    assert rep["backend"] == "nccl"
    assert rep["calls"] == W.expected_calls("deterministic", rep["n_launches"]) and rep["n_launches"] == 4, rep
    print(f"RCCL, one rank: bits equal to the single-GPU deterministic operator: {rep['bits_equal_single_gpu']}")
    BITS["deterministic hunyuan RCCL world 1 H 4 bf16"] = {n: b for n, b in rep["bits_equal_single_gpu"].items() if n != "dscores"}
    _check("RCCL, one rank, backward (kernels vs torch 16-bit autograd)", "deterministic hunyuan H 4 bf16",
           {n: tuple(p) for n, p in rep["pairs"].items()})


# ---------------------------------------------------------------------------------------------------------------- record
def test_accuracy_summary_written():
    """7: the figures of this module's cases (runs after them)"""
    if not FIGURES:
        return
    lines = []
    for kind in dict.fromkeys(f[0] for f in FIGURES):
        lines.append(kind + ": error / yardstick error (bound: 2)")
        for _, case, name, e, e_y in (f for f in FIGURES if f[0] == kind):
            lines.append(f"  {case} {name}: {e:.3e} / {e_y:.3e} = {e / max(e_y, 1e-300):.3f}")
    lines.append("deterministic: every rank's dq, dk, dv and dscores equal bit for bit across the backward passes of one forward:")
    lines += [f"  {case}: {n} passes, {'yes' if ok else 'NO'}" for case, (n, ok) in REPEATS.items()]
    lines.append("assembled dq, dk, dv bits equal to the single-process operator's under the same algorithm (a figure, not a claim):")
    lines += [f"  {case}: " + ", ".join(f"{n} {'yes' if b else 'no'}" for n, b in bits.items()) for case, bits in BITS.items()]
    print("\n".join(lines))
    path = os.environ.get("VORTA_SP_BACKWARD_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("tests/test_hip_sp_soft_mixture_backward.py: gloo ranks sharing one MI355X (host-staged transport)\n"
                    + "\n".join(lines) + "\n")
