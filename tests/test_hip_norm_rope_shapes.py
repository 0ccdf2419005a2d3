"""vorta_qk_norm_rope at the head counts, token counts and layouts where its two kernels take another path, against the rounding
model of tests/_side_kernel_models.py (float64 on the rounded inputs, one rounding at the store, a derived bound per element).
Every call works on a view into a wider buffer filled with a canary pattern -- one extra head column, guard rows before
token_offset and after the range -- and every byte outside the call's rows and heads must come back bit-unchanged."""
import numpy as np
import pytest
import torch

import _side_kernel_models as M
from _util import dev

pytestmark = pytest.mark.gpu

CASES = [(a, c) for a in (False, True) for c in M.NORM_ROPE_CASES[a]]
IDS = [M.norm_rope_case_id(a, c) for a, c in CASES]
GUARD = 2  # rows of the buffer in front of the view, and behind the call's range
FIGURES = {}


def _buffer(x, off, layout):
    """the call's rows x (H,n,D) placed into a canary-filled buffer; returns (buffer, the (H, off+n+GUARD, D) view to pass, mask of
    the buffer's elements the call owns)"""
    H, n, D = x.shape
    rows = GUARD + off + n + GUARD
    shape = (H + 1, rows, D) if layout == "hsd" else (rows, H + 1, D)
    canary = (torch.arange(shape[0] * shape[1] * D, dtype=torch.int32) % 251 + 0x3c00).to(torch.int16).view(x.dtype).reshape(shape)
    buf = canary.clone()
    full = buf if layout == "hsd" else buf.permute(1, 0, 2)  # (H+1, rows, D)
    full[:H, GUARD + off: GUARD + off + n] = x
    owned = torch.zeros(shape, dtype=torch.bool)
    (owned if layout == "hsd" else owned.permute(1, 0, 2))[:H, GUARD + off: GUARD + off + n] = True
    return buf, owned


def _call(x, w, cos, sin, off, rope, across, layout, with_cos=True):
    """run the kernel on x's rows inside the guarded buffer; returns (the rows after the call (H,n,D) float64, buffer bits before,
    buffer bits after, owned mask)"""
    from vorta_amd import ops
    H, n, D = x.shape
    buf, owned = _buffer(x, off, layout)
    before = buf.view(torch.int16).clone()
    d = buf.to(dev())
    full = d if layout == "hsd" else d.permute(1, 0, 2)
    view = full[:H, GUARD:]  # (H, off + n + GUARD, D): the guard rows behind the range are inside the view
    kw = dict(cos=cos.to(dev()), sin=sin.to(dev()), rope_tokens=rope) if with_cos else {}
    ops.qk_norm_rope(view, None if w is None else w.to(dev()), M.NORM_ROPE_EPS, n_tokens=n, token_offset=off,
                     across_heads=across, **kw)
    torch.cuda.synchronize()
    after = d.cpu()
    got = (after if layout == "hsd" else after.permute(1, 0, 2))[:H, GUARD + off: GUARD + off + n].double().numpy()
    return got, before, after.view(torch.int16), owned


def _check(got, x, w, cos, sin, rope, across, dtype):
    as64 = lambda t: None if t is None else t.double().numpy()
    ref, mag = M.norm_rope_model(as64(x), as64(w), M.NORM_ROPE_EPS, as64(cos), as64(sin), rope, across)
    assert np.isfinite(got).all()
    r = np.abs(got - ref) / M.norm_rope_bound(ref, mag, got, x.shape[0], across, dtype)
    return r, ref


@pytest.mark.parametrize("across,case", CASES, ids=IDS)
def test_norm_rope_case(across, case):
    dtype, H, n, off, rope, weight, layout = case
    x, w, cos, sin = M.norm_rope_inputs(across, case)
    got, before, after, owned = _call(x, w, cos, sin, off, rope, across, layout)
    assert torch.equal(after[~owned], before[~owned]), "bytes outside the call's rows and heads changed"
    r, _ = _check(got, x, w, cos, sin, rope, across, dtype)
    FIGURES[M.norm_rope_case_id(across, case)] = float(r.max())
    print(f"norm+rope {M.norm_rope_case_id(across, case)}: worst error / bound {r.max():.3f}")
    assert r.max() <= 1, np.argwhere(r > 1)[:8]
    assert not torch.equal(after[owned], before[owned])


@pytest.mark.parametrize("across", [False, True])
def test_no_rotation_table_is_rope_tokens_zero(across):
    """cos = sin = NULL: every row is normalised and none rotated, the bits of rope_tokens = 0"""
    case = M.NORM_ROPE_CASES[across][1]
    dtype, H, n, off, rope, weight, layout = case
    x, w, cos, sin = M.norm_rope_inputs(across, case)
    a = _call(x, w, cos, sin, off, 0, across, layout)
    b = _call(x, w, cos, sin, off, 0, across, layout, with_cos=False)
    assert torch.equal(a[2], b[2]) and torch.equal(b[2][~b[3]], b[1][~b[3]])
    r, _ = _check(b[0], x, w, None, None, 0, across, dtype)
    assert r.max() <= 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=M.dtype_name)
@pytest.mark.parametrize("across", [False, True])
def test_special_rows(across, dtype):
    """an all-zero row gives exact zeros, not NaN; a row of fp16 subnormals / bf16 1e-20 is dominated by eps and still meets the
    bound; a one-hot row; an fp16 row of +-3e4 in every channel (sum of squares ~1e11 per head, which fp32 holds) is finite and
    inside the bound"""
    x = M.special_rows(across, dtype)
    H, n, _ = x.shape
    w, cos, sin = M.norm_rope_inputs(across, (dtype, H, n, 0, n, True, "shd"))[1:]
    got, before, after, owned = _call(x, w, cos, sin, 3, n, across, "shd")
    assert torch.equal(after[~owned], before[~owned])
    r, ref = _check(got, x, w, cos, sin, n, across, dtype)
    zero = (x == 0).all(-1).numpy()
    assert zero.any() and not got[zero].any()
    FIGURES[f"{'across' if across else 'per_head'}-{M.dtype_name(dtype)}-special-rows"] = float(r.max())
    print(f"norm+rope special rows across={across} {M.dtype_name(dtype)}: worst error / bound {r.max():.3f}")
    assert r.max() <= 1, np.argwhere(r > 1)[:8]
    tiny = (x.double().abs().amax(-1) < 1e-4).numpy() & ~zero
    assert tiny.any() and (np.abs(ref[tiny]).max() < 0.2) and np.abs(got[tiny]).max() > 0  # eps-dominated, and not flushed


def test_across_heads_refuses_41_heads():
    from vorta_amd import _C, ops
    x = torch.zeros((41, 4, 128), dtype=torch.bfloat16, device=dev())
    with pytest.raises(_C.VortaHipError):
        ops.qk_norm_rope(x, None, 1e-6, across_heads=True)
    torch.cuda.synchronize()
    assert not x.any()


def test_accuracy_summary_written():
    """worst error / bound per case (runs after them; the norm+RoPE section of profiles/side_kernels_accuracy.txt comes from here
    when VORTA_SIDE_KERNELS_ACCURACY_OUT names a file)"""
    if not FIGURES:
        return  # (selected on its own: nothing to summarise)
    lines = [f"norm+rope {name}: error / bound {r:.4f}" for name, r in FIGURES.items()]
    M.write_record_section("norm+RoPE forward (tests/test_hip_norm_rope_shapes.py)", lines)
    assert all(r <= 1 for r in FIGURES.values())
