"""GPU: the routed output's fidelity under sequence parallelism -- `sp_attention(..., fidelity=[...])` and
`gather_routed_fidelity` on gloo ranks that share the one GPU (fresh child processes, at most 4, joined under one time limit:
`_run` of tests/test_hip_sp_soft_mixture.py) and on one rank with a real RCCL group (a child process under its own timeout).
Shapes: tests/_sp_soft_mixture.py (latent (12, 6, 8), S = 576; Hunyuan 8 text rows with 5 valid), 64 sampled rows; worker:
tests/_routed_fidelity_sp_worker.py.

A rank measures its local heads through the receive layout (the sampled rows composed with the row map) and files them under
their global ids; the gather takes every head from the rank that holds it.  Against the single-process call on the same
tensors, table and routes the sums are held to the chain bound (the header's chain for n = 64, not fitted):
    |sp - one| <= CHAIN(n) 2^-24 one
and the maxima are exact.  (Two float32 evaluations of one exact value in DIFFERENT orders could be twice that apart; here the
order is the same -- the compare reduces by sample position, not by physical row, and the reference launch cuts its keys by
the key count alone -- so the bits are in fact equal, which the test prints.)  Heads under the `split` placement stay NaN.
Under an 8-bit precision `sp_attention(fidelity=...)` refuses by name, before anything is exchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _routed_fidelity_sp_worker as W
from test_hip_sp_soft_mixture import ROOT, _free_port, _run

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (world, model, dtype, experts, placement, heads): even heads, uneven heads (H = 3 on 2 ranks), and a split full head
# (a rank start costs more than the case: one case per property, both models and both dtypes over the cases)
CASES = {"w2h4_hunyuan": (2, "hunyuan", "bf16", [0, 1, 2, 1], "auto", "all"),
         "w2h3_uneven_wan_sparse": (2, "wan", "fp16", [2, 0, 1], "auto", "sparse"),
         "w2h4_split_wan": (2, "wan", "bf16", [0, 2, 2, 2], "split", "all")}


def _compare(got, one, experts, heads, split, case):
    from vorta_amd import _C
    H = len(experts)
    chain = _C.sampled_fidelity_chain(W.N_ROWS)
    bound = chain * U
    assert bound < 1e-4
    assert got["expert"] == list(experts) == one["expert"]
    want = [h for h, e in enumerate(experts) if (e != 0 or heads == "all")]
    assert np.isfinite(one["sq_err"]).nonzero()[0].tolist() == want
    measured = [h for h in want if h not in split]
    for name in W.FIELDS:
        g = np.asarray(got[name], dtype=np.float64)
        assert g.shape == (H,) and np.isfinite(g).nonzero()[0].tolist() == measured, (case, name, g)
        assert np.isnan(g[[h for h in range(H) if h not in measured]]).all()
    for name in ("sq_ref", "sq_err"):
        g, o = (np.asarray(x[name], dtype=np.float64)[measured] for x in (got, one))
        assert (g[o == 0] == 0).all()  # (a full-attention head in the input dtype: the dense kernel twice, the same bits)
        g, o = g[o > 0], o[o > 0]
        ratio = np.abs(g - o) / (bound * o)
        print(f"{case} {name}: chain {chain}, bound {bound:.3e}, largest difference / bound {ratio.max():.4f}, "
              f"bits equal: {bool((g == o).all())}")
        assert (ratio <= 1.0).all(), (case, name, ratio)
    for name in ("max_ref", "max_err", "range_ref"):
        g, o = (np.asarray(x[name], dtype=np.float64)[measured] for x in (got, one))
        assert np.array_equal(g, o), (case, name)  # exact


@pytest.mark.parametrize("case", list(CASES))
def test_gathered_statistics_equal_the_single_process_ones(case):
    world, model, dtype, experts, placement, heads = CASES[case]
    H = len(experts)
    res = _run(W.routed_worker, world, (model, H, dtype, experts, placement, heads))["res"]
    held = []
    for r in res["per_rank"]:
        assert r["n_filed"] == 1 and r["shape"] == (H,) and r["n"] == W.N_ROWS * 128
        assert r["out_same"], "with fidelity=[...] the exchange and the routed output must keep their bits"
        held += r["local_heads"]
    assert sorted(set(held)) == list(range(H))  # every head is held somewhere, under its global id
    assert res["n"] == (W.N_ROWS * 128,) * 2 and res["rows"][0] == res["rows"][1] and len(res["rows"][0]) == W.N_ROWS
    if H % world:  # uneven heads: the ranks hold different numbers of them
        assert sorted(res["per_rank"][0]["counts"]) == [1, 2]
    if placement == "split":
        assert res["per_rank"][0]["taken"] == "split" and res["split"] == [0], res["split"]  # the full head is cut
        assert len(held) > H  # ... and held by more than one rank
    else:
        assert res["split"] == []
    _compare(res["got"], res["one"], experts, heads, res["split"], case)


def test_real_rccl_group_of_one_rank():
    """the direct branch of the exchange (all_to_all_single on RCCL's stream) and the gather's all_gather on device tensors"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0",
               VORTA_SP_FORCE_COLLECTIVES="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_routed_fidelity_sp_worker.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines and r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.loads(lines[-1])
    assert rep["backend"] == "nccl" and rep["mine"]["out_same"] and rep["mine"]["local_heads"] == [0, 1, 2, 3]
    # q, k, v in + o back, twice (without and with the sink); one all-gather per statistic and one for the expert ids
    assert rep["collective_calls"].get("all_to_all_single", 0) >= 8, rep["collective_calls"]
    assert rep["collective_calls"].get("all_gather", 0) >= 6, rep["collective_calls"]
    _compare(rep["got"], rep["one"], [0, 1, 2, 1], "all", rep["split"], "RCCL, one rank")


@pytest.mark.parametrize("precision", ["i8pv", "fp8pv", "auto8"])
def test_an_8_bit_precision_is_refused_by_name(monkeypatch, precision):
    """under an 8-bit precision v crosses the links as e4m3: the 16-bit reference cannot be formed on a rank, and the call says
    so before anything is exchanged or launched (in this process: a sequence-parallel group of one)"""
    import torch
    import _sp_soft_mixture as C
    import vorta_amd.attention._sp as sp
    import vorta_amd.routed as rt
    T, te = C.text_of("wan")
    q, k, v, sc, _ = C.operator_case("wan", 3, torch.bfloat16)
    kw = dict(C.geometry_kw(), model="wan", text_valid=te, experts_host=[0, 1, 2])
    monkeypatch.setattr(rt, "DEFAULT_FP8", precision)
    filed = []
    with pytest.raises(ValueError) as err:
        sp.sp_attention(q, k, v, T, sc, 0.0, fidelity=filed, fidelity_rows=W.N_ROWS, **kw)
    assert f"'{precision}'" in str(err.value) and "one GPU" in str(err.value) and filed == []
