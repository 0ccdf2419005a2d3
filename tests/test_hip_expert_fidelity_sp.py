"""GPU: the expert fidelity under sequence parallelism -- `sp_soft_mixture_attention[_autograd](..., fidelity=[...])` on gloo
ranks that share the one GPU (fresh child processes, at most 4, joined under one time limit: `_run` of
tests/test_hip_sp_soft_mixture.py).  Shapes and cases: tests/_sp_soft_mixture.py (latent (12, 6, 8), S = 576; Hunyuan 8 text
rows with 5 valid); worker: tests/_expert_fidelity_sp_worker.py.

A rank's kernel sees the (P + 1) Hl segments of S / P rows of its receive buffers and the host adds the P + 1 results of a
head; the ranks' heads are gathered over the group.  Against the single-process operator on the same tensors (whose expert
outputs are the same bits: profiles/sp_soft_mixture_accuracy.txt) the sums differ only by their summation order.  Bound (from
the header's chain, not fitted): both sums are within their own chain of the exact value E --
    |sp - one| <= (CHAIN(S / P) + P + CHAIN(S + T)) 2^-24 E,       E <= one / (1 - CHAIN(S + T) 2^-24)
-- and the maxima are exact.  Bit equality of the sums is not expected: the segments cut the rows differently."""
import numpy as np
import pytest

import _expert_fidelity_sp_worker as W
from test_hip_sp_soft_mixture import _run

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = {"w2h4": (2, 4), "w4h4": (4, 4), "w2h3_uneven": (2, 3)}
# every shape with both models (a rank start costs more than the case: one dtype each, both dtypes over the cases)
CASES = [("w2h4", "hunyuan", "bf16"), ("w2h4", "wan", "fp16"), ("w4h4", "hunyuan", "fp16"), ("w4h4", "wan", "bf16"),
         ("w2h3_uneven", "hunyuan", "bf16"), ("w2h3_uneven", "wan", "fp16")]


@pytest.mark.parametrize("shape,model,dtype", CASES, ids=["-".join(c) for c in CASES])
def test_gathered_statistics_equal_the_single_process_ones(shape, model, dtype):
    from vorta_amd import _C
    world, H = SHAPES[shape]
    res = _run(W.fidelity_worker, world, (model, H, dtype))["res"]
    counts = [2, 1] if H == 3 else [H // world] * world
    starts = np.concatenate([[0], np.cumsum(counts)])
    for rank, r in enumerate(res["per_rank"]):
        hl = counts[rank]
        assert tuple(r["heads"]) == (starts[rank], starts[rank + 1])  # this rank's heads [h0, h1)
        assert r["n_filed"] == (1, 1) and r["is_fidelity"]
        assert r["local_shapes"] == [(hl,), (hl,), (hl, 3), (hl, 3)]
        assert r["out_same"], "with fidelity=[...] the operator's output must keep its bits"
        assert r["grad_form_same"], "the differentiable form files the forward-only form's bits"
        assert r["grads_finite"]
    seg_rows, rows = res["rows"]
    assert res["n"] == (rows * 128, rows * 128)
    c_sp, c_one = _C.fidelity_chain(seg_rows) + world, _C.fidelity_chain(rows)
    bound = (c_sp + c_one) * U / (1.0 - c_one * U)
    assert bound < 1e-4
    got, one = res["got"], res["one"]
    for name in ("sq_ref", "sq_err"):
        g, o = got[name].astype(np.float64), one[name].astype(np.float64)
        assert g.shape == o.shape == ((H,) if name == "sq_ref" else (H, 3))
        assert np.isfinite(o).all() and (o > 0).all()
        ratio = np.abs(g - o) / (bound * o)
        print(f"{shape} {model} {dtype} {name}: chains {c_sp} + {c_one}, bound {bound:.3e}, largest difference / bound {ratio.max():.4f}")
        assert (ratio <= 1.0).all(), (name, ratio)
    for name in ("max_ref", "max_err"):
        assert np.array_equal(got[name], one[name]), name  # exact
