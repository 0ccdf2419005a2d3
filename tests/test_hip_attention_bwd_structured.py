"""GPU: the three attention-backward algorithms -- query_major (vorta_attn_bwd), key_major (vorta_attn_bwd_stats +
vorta_attn_bwd_kmajor) and deterministic (stats + vorta_attn_bwd_dq + vorta_attn_bwd_dkv) -- on the inputs training will see,
held to their own rounding model (tests/_attn_bwd_model.py) instead of torch's 16-bit autograd.

Inputs: white noise, peaked local heads, redundant heads with tied scores, score rows +-100 from zero, keys that lift the
running maximum late (by a little, by a lot, to P = 1), cotangents with a common part; bf16 and fp16; a dense launch and two
gather launches with tables, groups, duplicate rows and device lengths.  Rule, per gradient and algorithm, errors relative
Frobenius against float64:

    e_hip <= 2 e_model + 4 e_f32

e_model: float64 everywhere but the three roundings to 16 bits the kernels make by design (dO_eff, P, dS) -- the factor 2 of
tests/test_hip_attention_bwd.py, "same size" against "wrong".  e_f32: torch float32 autograd, for the kernels' float32 scores
and exp2 chain; tests/test_host_backward_model.py holds it under e_model / 4 on every case here, so the term adds at most one
e_model.  Torch's 16-bit autograd, the yardstick of the other backward tests, is 2-5 x the model on white noise, up to 50 x on
peaked rows and up to 120 x on shifted ones.  A gradient whose float64 norm is 0 must be exactly 0, and so must every row
the launch does not name.

Statistics (launches with a do_scale): delta by the same rule; lse2 ln 2 against float64 logsumexp per row within
2^-24 ((D + 2) scale max_j sum_d |q_d k_jd| + 8 max(|lse|, 1)): the forward error bound of a float32 dot product of length D
(lse is 1-Lipschitz in the scores) plus a few ulps for exp and log -- derived, not measured.

Measured on an MI355X: profiles/attn_bwd_structured_accuracy.txt."""
import math
import os

import numpy as np
import pytest
import torch

import _attn_bwd_model as M
from _attn_restate import named_rows
from _util import dev

pytestmark = pytest.mark.gpu

ALGORITHMS = ("query_major", "key_major", "deterministic")
GRADS = ("dq", "dk", "dv")
RATIOS = {}  # (family, dtype name, quantity, algorithm) -> list of (e_hip / e_model, e_model / e_torch16)
LSE = {}  # (family, dtype name, algorithm) -> list of the largest error / bound over the rows of a case


def _run(algorithm, q, k, v, out, d_o, bufs, w, kw):
    """one algorithm into bufs = [dq, dk, dv]; returns the statistics (None for query_major)"""
    from vorta_amd import ops
    if algorithm == "query_major":
        ops.attn_bwd(q, k, v, out, d_o, *bufs, do_scale=w, **kw)
        return None
    stats = ops.attn_bwd_stats(q, k, v, out, d_o, do_scale=w, **kw)
    if algorithm == "key_major":
        ops.attn_bwd_key_major(q, k, v, out, d_o, *bufs, stats, do_scale=w, **kw)
    else:
        ops.attn_bwd_dq(q, k, v, out, d_o, bufs[0], stats, do_scale=w, **kw)
        ops.attn_bwd_dkv(q, k, v, out, d_o, bufs[1], bufs[2], stats, do_scale=w, **kw)
    return stats


def _rule(what, quantity, key, e_hip, e_model, e_f32, e_t16):
    print(f"{what} {quantity}: e_hip {e_hip:.3e} e_model {e_model:.3e} e_f32 {e_f32:.3e} e_hip / e_model "
          f"{e_hip / max(e_model, 1e-300):.3f} e_model / e_torch16 {e_model / max(e_t16, 1e-300):.4f}")
    RATIOS.setdefault(key, []).append((e_hip / max(e_model, 1e-300), e_model / max(e_t16, 1e-300)))
    assert e_hip <= 2.0 * e_model + 4.0 * e_f32, \
        f"{what} {quantity}: e_hip {e_hip:.3e} > 2 x e_model {e_model:.3e} + 4 x e_f32 {e_f32:.3e}"


@pytest.mark.parametrize("which", M.LAUNCHES)
@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.dtype_name)
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_structured_inputs(fam, dtype, which):
    from vorta_amd import ops
    c = M.case(fam, dtype, which)  # the references: computed once on the CPU, never from the library
    H, S, kw, weighted = M.launch(which, dev())
    shape = (H, S, 128)
    q, k, v, d_o = (c[n].to(dev()) for n in ("q", "k", "v", "d_o"))
    w = c["w"].to(dev()) if weighted else None
    out = torch.zeros(shape, dtype=dtype, device=dev())
    ops.attn_fwd(q, k, v, out, **kw)
    errs = M.rel_errors(c)
    qm, km = named_rows(c["kw"], shape)
    dn = M.dtype_name(dtype)
    for algorithm in ALGORITHMS:
        what = f"{fam} {dn} {which} {algorithm}"
        bufs = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
        stats = _run(algorithm, q, k, v, out, d_o, bufs, w, kw)
        for i, name in enumerate(GRADS):
            got = bufs[i].cpu()
            assert torch.isfinite(got).all(), f"{what}: {name} is not finite"
            untouched = ~(qm if name == "dq" else km)
            assert not c["f64"][i][untouched].any()  # (the references agree on which rows those are)
            assert not got[untouched].any(), f"{what}: {name} wrote rows the launch does not name"
            if errs[name] is None:
                assert not got.any(), f"{what}: {name} must be exactly zero"
                continue
            e_hip = M.fro(got.double() - c["f64"][i]) / M.fro(c["f64"][i])
            _rule(what, name, (fam, dn, name, algorithm), e_hip, *errs[name])
        if stats is None or not weighted:
            continue
        # ---- the statistics both stats-based algorithms start from
        stats = stats.double().cpu()
        lse64, delta64 = c["f64"][3], c["f64"][4]
        covered = ~torch.isnan(lse64)
        assert covered.any() and tuple(stats.shape[1:]) == (kw["n_q"], 2) and stats.shape[0] >= covered.shape[0]
        stats = stats[: covered.shape[0]]
        n = M.fro(delta64[covered])
        e_hip, e_model, e_f32 = (M.fro(x[covered] - delta64[covered]) / n for x in (stats[..., 1], c["model"][4], c["f32_delta"]))
        _rule(what, "delta", (fam, dn, "delta", algorithm), e_hip, e_model, e_f32, float("nan"))
        lse_hip = stats[..., 0] * math.log(2.0)
        scale = kw.get("scale") or 1.0 / math.sqrt(128)
        bound = 2.0 ** -24 * ((128 + 2) * scale * c["abs_sums"] + 8.0 * lse64.abs().clamp(min=1.0))
        err = (lse_hip - lse64).abs()
        worst = (err[covered] / bound[covered]).max()
        print(f"{what} lse: max error {err[covered].max():.3e}, at most {worst:.3f} of the row's bound")
        LSE.setdefault((fam, dn, algorithm), []).append(float(worst))
        assert torch.isfinite(lse_hip[covered]).all() and worst <= 1.0, \
            f"{what}: lse2 ln 2 is {err[covered].max():.3e} from float64 logsumexp, {worst:.2f} x the float32 bound of its row"


def test_accuracy_summary_written():
    """max / median of e_hip / e_model and of e_model / e_torch16 per (family, dtype, quantity, algorithm) over this module's
    cases (runs after them; profiles/attn_bwd_structured_accuracy.txt comes from here when
    VORTA_BWD_STRUCTURED_ACCURACY_OUT names a file)"""
    if not RATIOS:
        return  # (selected on its own: nothing to summarise)
    lines = []
    for (fam, dn, name, alg), r in sorted(RATIOS.items()):
        hip, t16 = np.array([a for a, _ in r]), np.array([b for _, b in r])
        line = f"{fam} {dn} {name} {alg}: cases {len(r)} e_hip / e_model max {hip.max():.3f} median {float(np.median(hip)):.3f}"
        if name in GRADS:
            line += f"  e_model / e_torch16 max {t16.max():.4f} median {float(np.median(t16)):.4f}"
        lines.append(line)
    lines += [f"{fam} {dn} lse {alg}: cases {len(r)} error / bound of the row max {max(r):.3f}" for (fam, dn, alg), r in sorted(LSE.items())]
    for alg in ALGORITHMS:  # the figures of DESIGN.md 6.8
        for dn in map(M.dtype_name, M.DTYPES):
            r = np.array([a for (f, d, name, al), rs in RATIOS.items() if al == alg and d == dn and name in GRADS for a, _ in rs])
            if len(r):
                lines.append(f"all families {dn} dq/dk/dv {alg}: cases {len(r)} e_hip / e_model max {r.max():.3f} "
                             f"median {float(np.median(r)):.3f}")
    print("\n".join(lines))
    path = os.environ.get("VORTA_BWD_STRUCTURED_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / e_model of the three attention-backward algorithms over the cases of "
                    "tests/test_hip_attention_bwd_structured.py (rule: e_hip <= 2 e_model + 4 e_f32), and how far under "
                    "torch's 16-bit autograd the model sits\n" + "\n".join(lines) + "\n")
