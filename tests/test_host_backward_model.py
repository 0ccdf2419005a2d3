"""CPU-only: the rounding model of the attention backward (tests/_attn_bwd_model.py) is checked itself before any kernel is held
to it (tests/test_hip_attention_bwd_structured.py).

  * without its roundings it IS the attention backward: float64 autograd through the restatement of tests/_attn_restate.py, on
    random launches with tables, groups, duplicate rows, q_valid and device lengths, to 1e-12;
  * the cap: on every input family, dtype and launch the structured tests use, the error of float32 autograd is at most a
    quarter of the model's error, so the float32 term of their rule, 4 e_f32, adds at most one e_model.  A condition on the
    families, not a measurement: a family that leaves the cap is changed, the cap is not;
  * every reference is finite on every family."""
import math

import numpy as np
import pytest
import torch

import _attn_bwd_model as M
import _random_launch as RL

GRADS = ("dq", "dk", "dv")


@pytest.mark.parametrize("seed", range(24))
def test_model_without_roundings_is_float64_autograd(seed):
    rng = np.random.default_rng(3000 + seed)
    L = RL.draw(rng, S_range=(64, 300), H_max=3)
    kw = RL.kwargs(L, "cpu")
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dtype = M.DTYPES[seed % 2]
    q, k, v, d_o = (torch.randn((L.H_buf, L.S, 128), generator=gen).to(dtype) for _ in range(4))
    w = torch.randn(L.H_buf, generator=gen).to(dtype) if seed % 4 < 2 else None
    got = M.model_grads(kw, q, k, v, d_o, w, dtype, round16=False)
    want = M.autograd_grads(kw, q, k, v, d_o, w, torch.float64)
    for name, a, b in zip(GRADS, got, want):
        n = M.fro(b)
        if n == 0.0:
            assert not a.any(), f"seed {seed} {name}: the float64 gradient is zero, the model's is not"
            continue
        e = M.fro(a - b) / n
        assert e <= 1e-12, f"seed {seed} {RL.describe(L)} {name}: model without roundings is {e:.3e} from float64 autograd"


def test_the_random_launches_reach_every_feature():
    """(so the test above pins what it claims to pin)"""
    seen = set()
    for seed in range(24):
        L = RL.draw(np.random.default_rng(3000 + seed), S_range=(64, 300), H_max=3)
        if len(L.live) == 0 or L.q_valid_eff == 0:
            continue  # nothing flows: the gradient is zero
        seen.add(L.mode)
        seen.update(name for name, on in (("dup", L.n_dup_pos > 0), ("q_rows", L.q_rows is not None),
                                          ("kv_rows", L.kv_rows is not None), ("q_valid", L.q_valid_eff < L.n_q),
                                          ("n_kv_dev", L.n_kv_eff < L.n_kv), ("head_list", len(L.live) < L.H_buf)) if on)
    assert seen >= {"one", "equal", "table", "dup", "q_rows", "kv_rows", "q_valid", "n_kv_dev", "head_list"}, seen


@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.dtype_name)
def test_each_rounding_of_the_model_by_hand(dtype):
    """three keys with scores 0 (q = e_5, k_j = e_j), v_j = j e_0, d_o = g0 e_0 on two query rows and a weight w: then
    P = 1/3, g = round16(g0 w), dP_ij = g j, delta = g, dS_ij = g (j - 1) / 3, and with p16 = round16(1/3), s16 = round16(g / 3):
    dv_j = 2 p16 g e_0, dq_i = scale s16 (e_2 - e_0), dk_j = 2 scale (j - 1) s16 e_5.  Each of the three roundings shows: g0 w,
    1/3 and g / 3 are no 16-bit numbers."""
    r16 = lambda x: float(torch.tensor(x, dtype=torch.float64).to(dtype))  # noqa: E731
    eps = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    g0, w0 = 1 + eps, 1 + 2 * eps  # 16-bit numbers whose product is none
    q, k, v, d_o = (torch.zeros((1, 8, 128), dtype=dtype) for _ in range(4))
    q[0, :2, 5] = 1
    for j in range(3):
        k[0, j, j], v[0, j, 0] = 1, j
    d_o[0, :2, 0] = g0
    w = torch.tensor([w0], dtype=dtype)
    assert float(d_o[0, 0, 0]) == g0 and float(w[0]) == w0 and r16(g0 * w0) != g0 * w0
    scale = 128 ** -0.5
    for rounded in (True, False):
        rr = r16 if rounded else (lambda x: x)
        g = rr(g0 * w0)
        p16, s16 = rr(1 / 3), rr(g / 3)
        assert not rounded or (p16 != 1 / 3 and s16 != g / 3)
        dq, dk, dv, lse, delta = M.model_grads(dict(n_q=2, n_kv=3), q, k, v, d_o, w, dtype, round16=rounded)
        want_dq, want_dk, want_dv = (torch.zeros((1, 8, 128), dtype=torch.float64) for _ in range(3))
        want_dq[0, :2, 0], want_dq[0, :2, 2] = -scale * s16, scale * s16
        want_dk[0, 0, 5], want_dk[0, 2, 5] = -2 * scale * s16, 2 * scale * s16
        want_dv[0, :3, 0] = 2 * p16 * g
        for name, a, b in zip(GRADS, (dq, dk, dv), (want_dq, want_dk, want_dv)):
            assert torch.allclose(a, b, rtol=1e-12, atol=1e-15), f"{name} round16={rounded}: {a[a != b]} against {b[a != b]}"
        assert torch.allclose(lse, torch.full((1, 2), math.log(3.0), dtype=torch.float64), rtol=1e-14, atol=0)
        assert torch.allclose(delta, torch.full((1, 2), g, dtype=torch.float64), rtol=1e-14, atol=0)


@pytest.mark.parametrize("which", M.LAUNCHES)
@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.dtype_name)
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_cap_float32_error_is_a_quarter_of_the_models(fam, dtype, which):
    c = M.case(fam, dtype, which)
    for x in c["f64"][:3] + c["model"][:3] + tuple(c["f32"]):
        assert torch.isfinite(x).all(), f"{fam} {M.dtype_name(dtype)} {which}: a reference gradient is not finite"
    for x in (c["f64"][3], c["f64"][4], c["model"][3], c["model"][4], c["f32_delta"]):
        assert torch.isfinite(x[~torch.isnan(c["f64"][3])]).all()
    for name, e in M.rel_errors(c).items():
        assert e is not None, f"{fam} {which} {name}: the launch gives no gradient"
        e_model, e_f32, e_t16 = e
        print(f"{fam} {M.dtype_name(dtype)} {which} {name}: e_model {e_model:.3e} e_f32 {e_f32:.3e} "
              f"e_f32 / e_model {e_f32 / e_model:.4f} e_torch16 / e_model {e_t16 / e_model:.1f}")
        assert e_model > 0.0
        assert e_f32 <= e_model / 4, f"{fam} {M.dtype_name(dtype)} {which} {name}: e_f32 {e_f32:.3e} > e_model / 4 = {e_model / 4:.3e}"


def test_the_families_are_what_they_are_meant_to_be():
    """peaked rows, tied scores, scores +-100 from zero, a late key that lifts the maximum, a cotangent with a common part"""
    scale = 128 ** -0.5
    s = lambda q, k: (q[0].double() @ k[0].double().t()) * scale  # noqa: E731
    q, k, v, d_o = M.family("white", 1, M.S_VID, torch.bfloat16)
    assert torch.softmax(s(q, k), -1).max(-1).values.median() < 0.1
    q, k, v, d_o = M.family("local", 1, M.S_VID, torch.bfloat16)
    assert torch.softmax(s(q, k), -1).max(-1).values.median() > 0.5
    q, k, v, d_o = M.family("redundant", 1, M.S_VID, torch.bfloat16)
    top2 = torch.softmax(s(q, k), -1).topk(2, dim=-1).values
    assert (top2[:, 1] / top2[:, 0]).median() > 0.5  # the duplicates of the best key score nearly the same
    q, k, v, d_o = M.family("shift_up", 1, M.S_VID, torch.float16)
    assert s(q, k).mean() > 90
    q, k, v, d_o = M.family("shift_down", 1, M.S_VID, torch.float16)
    assert s(q, k).mean() < -90
    q, k, v, d_o = M.family("late_key", 1, M.S_VID, torch.float16)
    sc = s(q, k)
    for row, key, b in M.LATE_KEYS:
        assert b < 0.5 or sc[row].argmax() == key  # (b = 1/4 lifts the key to the row's crowd of maxima, not above it)
    p = torch.softmax(sc[77], -1)
    assert p.to(torch.float16)[383] == 1.0 and sc[77, 383] - sc[77, :383].max() > 20  # P = 1, and the maximum rises last
    q, k, v, d_o = M.family("common_cotangent", 1, M.S_VID, torch.bfloat16)
    assert abs(d_o.double().mean() - 4) < 0.1
