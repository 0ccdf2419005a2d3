"""The yardsticks of tests/_side_kernel_models.py, checked without a GPU: with the roundings off they are the oracle; an fp32
restatement of the kernels' arithmetic stays inside their bounds (the bounds are attainable), one that reads less than it should
does not (the bounds are tight enough to see it); and the routing-clarity condition holds on the router cases, decided on the
reference alone."""
import numpy as np
import pytest
import torch

import _side_kernel_models as M
from oracle import vorta_oracle as O

ROUTER = sorted(M.ROUTER_CASES)
NORM_ROPE = [(a, c) for a in (False, True) for c in M.NORM_ROPE_CASES[a]]
NORM_ROPE_IDS = [M.norm_rope_case_id(a, c) for a, c in NORM_ROPE]


def _np(*ts):
    return [None if t is None else t.double().numpy() for t in ts]


# ------------------------------------------------------------------------------------------------ the rounding helpers
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_T_is_the_dtype_conversion(dtype):
    """round_T against torch's own conversion on every finite value of T's neighbourhoods: midpoints (ties to even), subnormals,
    overflow"""
    bits = torch.arange(0, 0x7c00 if dtype == torch.float16 else 0x7f80, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype).double().numpy()
    assert np.array_equal(M.round_T(v, dtype), v)
    mid = (v[:-1] + v[1:]) / 2  # exact in float64
    want = torch.from_numpy(mid.astype(np.float32)).to(dtype).double().numpy()  # (a midpoint of T is exact in fp32)
    assert np.array_equal(M.round_T(mid, dtype), want)
    assert np.array_equal(M.round_T(-mid * (1 + 2.0 ** -30), dtype), -v[1:])
    assert np.array_equal(M.ulp_T(v[:-1], dtype), v[1:] - v[:-1])
    assert np.isinf(M.round_T(v[-1] * 1.01, dtype)) and M.round_T(-0.0, dtype) == 0


# ------------------------------------------------------------------------------------------------ router
@pytest.mark.parametrize("case", ROUTER)
def test_router_model_without_roundings_is_the_oracle(case):
    dtype, B, E, H = M.ROUTER_CASES[case]
    temb, W, b = _np(*M.router_inputs(case))
    m = M.router_model(temb, W, b, H, dtype, roundings=False)
    assert np.abs(m.scores64 - O.router_scores(temb, W, b, H)).max() <= 1e-13


@pytest.mark.parametrize("case", ROUTER)
def test_router_restatement_inside_truncated_outside(case):
    """fp32 restatement: every logit within lb, every score within sb; with the last 8 elements of the dot product dropped at
    least one logit leaves lb"""
    dtype, B, E, H = M.ROUTER_CASES[case]
    temb, W, b = M.router_inputs(case)
    m = M.router_model(temb, W, b, H, dtype)
    f = [t.float().numpy() for t in (temb, W, b)]
    lg, sc = M.router_restate_f32(*f, H, dtype)
    rl = np.abs(lg - m.logit64) / m.logit_bound(lg)
    rs = np.abs(sc - m.scores64) / m.score_bound(lg)
    lt, _ = M.router_restate_f32(*f, H, dtype, drop_last=8)
    over = np.abs(lt - m.logit64) > m.logit_bound(lt)
    print(f"router {case}: restatement logit {rl.max():.3f} score {rs.max():.3f} of the bound; truncated: {over.mean():.2f} of the "
          "logits outside")
    assert rl.max() <= 1 and rs.max() <= 1
    assert over.any()
    assert np.isfinite(m.logit64).all() and np.isfinite(sc).all()
    if case == M.PLANTED_CASE:  # silu(-120) is (minus) zero in T, silu(120) = 120
        s = m.s[0, 1:1 + len(M.PLANTED)]
        assert s[0] == 120 and s[1] == 0 and s[4] == 0 and abs(s[3]) < 1e-7


@pytest.mark.parametrize("tau", M.ROUTER_TAUS)
@pytest.mark.parametrize("case", ROUTER)
def test_unclear_heads_within_the_cap(case, tau):
    """a head is clear when batch item 0's top score beats the runner-up by more than 2 max_e sb and lies more than that from
    round_T(tau); at most max(1, H/4) heads of a case may be unclear (decided on the reference alone)"""
    dtype, B, E, H = M.ROUTER_CASES[case]
    m = M.router_model(*M.router_inputs(case), H, dtype)
    unclear = int((~m.clear_heads(tau)).sum())
    print(f"router {case} tau {tau}: {unclear} of {H} heads unclear (cap {M.unclear_cap(H)})")
    assert unclear <= M.unclear_cap(H)
    # the bounds that need no kernel output are no smaller than the ones evaluated at an output inside them
    lg, _ = M.router_restate_f32(*[t.float().numpy() for t in M.router_inputs(case)], H, dtype)
    assert (m.lb_ref >= m.logit_bound(lg)).all() and (m.sb_ref >= m.score_bound(lg)).all()


# ------------------------------------------------------------------------------------------------ norm + RoPE
@pytest.mark.parametrize("across,case", NORM_ROPE, ids=NORM_ROPE_IDS)
def test_norm_rope_model_is_the_oracle(across, case):
    """the model is O.rms_norm then O.rope_interleaved on the rounded inputs, written out once more by hand"""
    dtype, H, n, off, rope, weight, layout = case
    x, w, cos, sin = _np(*M.norm_rope_inputs(across, case))
    ref, mag = M.norm_rope_model(x, w, M.NORM_ROPE_EPS, cos, sin, rope, across)
    eps = float(np.float32(M.NORM_ROPE_EPS))
    ms = (x * x).mean(axis=(0, 2), keepdims=True) if across else (x * x).mean(-1, keepdims=True)
    y = x / np.sqrt(ms + eps)
    if w is not None:
        y = y * (w.reshape(H, 1, 128) if across else w)
    want = y.copy()
    want[:, :rope, 0::2] = y[:, :rope, 0::2] * cos[:rope, 0::2] - y[:, :rope, 1::2] * sin[:rope, 0::2]
    want[:, :rope, 1::2] = y[:, :rope, 1::2] * cos[:rope, 1::2] + y[:, :rope, 0::2] * sin[:rope, 1::2]
    assert np.abs(ref - want).max() <= 1e-13
    assert (mag[:, rope:] == np.abs(y[:, rope:])).all() and (mag >= np.abs(ref) * (1 - 1e-12)).all()


@pytest.mark.parametrize("across,case", NORM_ROPE, ids=NORM_ROPE_IDS)
def test_norm_rope_restatement_inside_truncated_outside(across, case):
    """fp32 restatement inside the bound everywhere; one whose sum of squares skips the last head (across heads, more than one
    head) or the last 16-byte chunk of a row lands outside it"""
    dtype, H, n, off, rope, weight, layout = case
    x, w, cos, sin = M.norm_rope_inputs(across, case)
    xd, wd, cd, sd = _np(x, w, cos, sin)
    ref, mag = M.norm_rope_model(xd, wd, M.NORM_ROPE_EPS, cd, sd, rope, across)
    f = [None if t is None else t.float().numpy() for t in (x, w)]
    got = M.norm_rope_restate_f32(*f, M.NORM_ROPE_EPS, cos.numpy(), sin.numpy(), rope, across, dtype)
    r = np.abs(got - ref) / M.norm_rope_bound(ref, mag, got, H, across, dtype)
    skip = "head" if across and H > 1 else "chunk"
    bad = M.norm_rope_restate_f32(*f, M.NORM_ROPE_EPS, cos.numpy(), sin.numpy(), rope, across, dtype, skip=skip)
    over = np.abs(bad - ref) > M.norm_rope_bound(ref, mag, bad, H, across, dtype)
    print(f"norm+rope {M.norm_rope_case_id(across, case)}: restatement {r.max():.3f} of the bound; skipping the last {skip}: "
          f"{over.mean():.2f} of the elements outside")
    assert r.max() <= 1
    assert over.any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("across", [False, True])
def test_norm_rope_special_rows_restatement(across, dtype):
    """zero, eps-dominated, one-hot and (fp16) huge rows: the model is finite, zero rows give zeros, the fp32 restatement is
    inside the bound"""
    x = M.special_rows(across, dtype)
    H, n, _ = x.shape
    w, cos, sin = M.norm_rope_inputs(across, (dtype, H, n, 0, n, True, "hsd"))[1:]
    ref, mag = M.norm_rope_model(*_np(x, w), M.NORM_ROPE_EPS, *_np(cos, sin), n, across)
    got = M.norm_rope_restate_f32(x.float().numpy(), w.float().numpy(), M.NORM_ROPE_EPS, cos.numpy(), sin.numpy(), n, across, dtype)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    zero = (x == 0).all(-1).numpy()
    assert zero.any() and not ref[zero].any() and not got[zero].any()
    assert (np.abs(got - ref) <= M.norm_rope_bound(ref, mag, got, H, across, dtype)).all()


def test_norm_rope_slack():
    assert M.norm_rope_slack(24, False) == 14 * M.U32
    assert M.norm_rope_slack(1, True) == (14 / 2 + 8) * M.U32 and M.norm_rope_slack(40, True) == (86 / 2 + 8) * M.U32
