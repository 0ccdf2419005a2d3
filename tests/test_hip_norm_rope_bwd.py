"""GPU: vorta_qk_norm_rope_bwd (csrc/qk_norm_rope_bwd.hip) and its autograd wrappers against torch autograd in float64 on
the restatement of tests/_norm_rope_restate.py, fed the same 16-bit-rounded inputs.

Tolerance: the rule of the attention backward (tests/test_hip_attention_bwd.py, "bound 2").  Per case and output,
e_hip = rel_fro(kernel, f64) <= 2 x e_torch = rel_fro(torch 16-bit autograd of the same restatement, f64).  dweight is
compared as the kernel returns it (float32).  VORTA_NORM_ROPE_BWD_ACCURACY_OUT names a file that receives the ratios."""
import os

import numpy as np
import pytest
import torch

from _norm_rope_restate import grads, rel_err
from _util import dev

pytestmark = pytest.mark.gpu

EPS = 1e-6
RATIOS = {}


def _tables(S, gen):
    ang = torch.rand((S, 128), generator=gen) * 6.283  # four independent entries per pair: not a true rotation table
    ang2 = torch.rand((S, 128), generator=gen) * 6.283
    return torch.cos(ang).to(dev()), torch.sin(ang2).to(dev())


def _inputs(H, S, dtype, seed, weight="head", transposed=False):
    gen = torch.Generator(device="cpu").manual_seed(seed)

    def mk():
        if transposed:  # the (H,S,D) view of an (S, H*D) projection
            return (torch.randn((S, H * 128), generator=gen) * 1.5).to(dtype).to(dev()).view(S, H, 128).transpose(0, 1)
        return (torch.randn((H, S, 128), generator=gen) * 1.5).to(dtype).to(dev())

    x, g = mk(), mk()
    n = {"head": 128, "all": H * 128, None: 0}[weight]
    w = (1.0 + 0.3 * torch.randn(n, generator=gen)).to(dtype).to(dev()) if n else None
    return x, g, w, gen


def _bound(what, name, got, t16, ref):
    e_hip, e_t = rel_err(got, ref), rel_err(t16, ref)
    print(f"{what} {name}: e_hip {e_hip:.3e} e_torch {e_t:.3e} ratio {e_hip / max(e_t, 1e-300):.3f}")
    RATIOS.setdefault(name, []).append(e_hip / max(e_t, 1e-300))
    assert e_hip <= 2.0 * e_t, f"{what} {name}: e_hip {e_hip:.3e} > 2 x e_torch {e_t:.3e}"


def _check(what, x, g, w, cos, sin, rope_tokens, across, dx, dw, off=0, n=None):
    n = x.shape[1] - off if n is None else n
    xs, gs = x[:, off:off + n], g[:, off:off + n]
    ref = grads(xs, gs, w, EPS, cos, sin, rope_tokens, across, torch.float64)
    t16 = grads(xs, gs, w, EPS, cos, sin, rope_tokens, across, x.dtype)
    _bound(what, "dx", dx[:, off:off + n], t16[0], ref[0])
    if w is not None:
        _bound(what, "dweight", dw, t16[1], ref[1])
    else:
        assert dw is None


CASES = [  # (id, H, S, weight, across, tables, rope_tokens (None: all), transposed)
    ("head_all", 24, 37, "head", False, True, None, False),
    ("head_text_tail", 24, 37, "head", False, True, 21, False),
    ("head_rope0", 24, 37, "head", False, True, 0, False),
    ("head_no_tables", 24, 37, "head", False, False, None, False),
    ("head_no_weight", 24, 37, None, False, True, None, False),
    ("head_transposed", 24, 37, "head", False, True, 21, True),
    ("head_h3", 3, 13, "head", False, True, 9, False),
    ("across_h12", 12, 37, "all", True, True, None, False),
    ("across_h12_transposed", 12, 37, "all", True, True, 21, True),
    ("across_h24", 24, 30, "all", True, True, None, True),
    ("across_h40", 40, 37, "all", True, True, None, False),
    ("across_h40_text_tail", 40, 38, "all", True, True, 17, True),
    ("across_no_weight", 12, 37, None, True, False, None, False),
    ("across_h5", 5, 19, "all", True, True, None, False),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_against_float64(case, dtype):
    from vorta_amd import ops
    name, H, S, weight, across, tables, rt, transposed = case
    x, g, w, gen = _inputs(H, S, dtype, 7 + len(name), weight, transposed)
    cos, sin = _tables(S, gen) if tables else (None, None)
    dx = torch.empty_like(g)
    assert dx.stride() == g.stride()
    x0, g0 = x.clone(), g.clone()
    got, dw = ops.qk_norm_rope_bwd(x, g, w, EPS, cos=cos, sin=sin, rope_tokens=rt, across_heads=across, dx=dx)
    assert got is dx and torch.equal(x, x0) and torch.equal(g, g0)  # inputs are read only
    _check(f"{name} {dtype}", x, g, w, cos, sin, (S if rt is None else rt) if tables else 0, across, dx, dw)
    # without dweight: the same dx bits from the lean instantiation
    dx2, none = ops.qk_norm_rope_bwd(x, g, w, EPS, cos=cos, sin=sin, rope_tokens=rt, across_heads=across, want_dweight=False)
    assert none is None and torch.equal(dx2, dx)


@pytest.mark.parametrize("across", [False, True], ids=["head", "across"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_token_range_leaves_other_rows_untouched(across, dtype):
    """token_offset > 0 and n_tokens short of the end: rows outside the range keep the sentinel's bits; a second call
    covers the text range with its own weight, as the processors cover [video | text]"""
    from vorta_amd import ops
    H, S, off, n, rt = (12 if across else 24), 45, 6, 30, 19
    x, g, w, gen = _inputs(H, S, dtype, 3, "all" if across else "head", transposed=True)
    cos, sin = _tables(n, gen)
    sentinel = torch.full((S, H * 128), 777.0, dtype=dtype, device=dev()).view(S, H, 128).transpose(0, 1)
    dx = sentinel.clone()
    _, dw = ops.qk_norm_rope_bwd(x, g, w, EPS, cos=cos, sin=sin, n_tokens=n, token_offset=off, rope_tokens=rt,
                                 across_heads=across, dx=dx)
    assert torch.equal(dx[:, :off], sentinel[:, :off]) and torch.equal(dx[:, off + n:], sentinel[:, off + n:])
    _check(f"range {across} {dtype}", x, g, w, cos, sin, rt, across, dx, dw, off, n)
    # the default buffer is zero outside the range
    dz, _ = ops.qk_norm_rope_bwd(x, g, w, EPS, cos=cos, sin=sin, n_tokens=n, token_offset=off, rope_tokens=rt,
                                 across_heads=across)
    assert torch.equal(dz[:, off:off + n], dx[:, off:off + n]) and not dz[:, :off].any() and not dz[:, off + n:].any()
    with pytest.raises(ValueError):
        ops.qk_norm_rope_bwd(x, g, w, EPS, n_tokens=S, token_offset=1, across_heads=across)


@pytest.mark.parametrize("across", [False, True], ids=["head", "across"])
def test_dx_may_alias_g(across):
    from vorta_amd import ops
    H, S = (12 if across else 24), 41
    x, g, w, gen = _inputs(H, S, torch.bfloat16, 11, "all" if across else "head", transposed=across)
    cos, sin = _tables(S, gen)
    want, dw = ops.qk_norm_rope_bwd(x, g, w, EPS, cos=cos, sin=sin, across_heads=across)
    g2 = g.clone()
    got, dw2 = ops.qk_norm_rope_bwd(x, g2, w, EPS, cos=cos, sin=sin, across_heads=across, dx=g2)
    assert got is g2 and torch.equal(g2, want) and torch.equal(dw, dw2)


@pytest.mark.parametrize("across", [False, True], ids=["head", "across"])
def test_bit_identical_across_runs_with_many_workgroups(across):
    """more token groups than workgroups (the grid-stride walk), every workgroup's partial summed in a fixed order"""
    from vorta_amd import _C, ops
    H, S = (12 if across else 24), 4 * _C.NORM_ROPE_BWD_PARTS + 4 * 37 + 3
    dtype = torch.bfloat16
    x, g, w, gen = _inputs(H, S, dtype, 5, "all" if across else "head")
    cos, sin = _tables(S, gen)
    runs = [ops.qk_norm_rope_bwd(x, g, w, EPS, cos=cos, sin=sin, rope_tokens=S - 50, across_heads=across) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    _check(f"large {across}", x, g, w, cos, sin, S - 50, across, *runs[0])


def test_no_tokens_zeroes_dweight():
    from vorta_amd import ops
    x, g, w, _ = _inputs(24, 8, torch.float16, 2)
    sent = torch.full_like(g, 5.0)
    dx, dw = ops.qk_norm_rope_bwd(x, g, w, EPS, n_tokens=0, token_offset=3, dx=sent)
    assert (dx == 5.0).all() and dw.shape == (128,) and not dw.any()


# ---------------------------------------------------------------------------------------------------- autograd wrappers
@pytest.mark.parametrize("across", [False, True], ids=["head", "across"])
@pytest.mark.parametrize("via", ["function", "torch_op"])
def test_autograd_wrapper_is_the_two_ops(across, via):
    """16 bits rule torch.autograd.gradcheck out: the forward must be the in-place op on a copy, bit for bit, and the
    backward ops.qk_norm_rope_bwd"""
    from vorta_amd import ops, routed, torch_ops  # noqa: F401
    H, S, rt = (12 if across else 24), 29, 17
    dtype = torch.bfloat16
    x, g, w, gen = _inputs(H, S, dtype, 13, "all" if across else "head", transposed=True)
    cos, sin = _tables(S, gen)
    x4 = x[None].detach().requires_grad_(True)  # (1,H,N,D) transposed view, as the processors make it
    wl = w.detach().requires_grad_(True)
    if via == "function":
        y = routed.qk_norm_rope_autograd(x4, wl, EPS, cos, sin, rt, across)
    else:
        y = torch.ops.vorta.qk_norm_rope_grad(x4, wl, EPS, cos, sin, rt, across)
    want = x.clone()
    ops.qk_norm_rope(want, w, EPS, cos=cos, sin=sin, rope_tokens=rt, across_heads=across)
    assert y.is_contiguous() and torch.equal(y[0], want) and torch.equal(x4[0], x)  # out of place
    gc = g.contiguous()
    dx, dw = torch.autograd.grad(y, [x4, wl], gc[None])
    wdx, wdw = ops.qk_norm_rope_bwd(x, gc, w, EPS, cos=cos, sin=sin, rope_tokens=rt, across_heads=across)
    assert torch.equal(dx[0], wdx) and torch.equal(dw, wdw.to(dtype)) and dw.shape == w.shape
    # a frozen weight: no dweight is computed, dx keeps its bits
    y = routed.qk_norm_rope_autograd(x4, w, EPS, cos, sin, rt, across)
    (dx2,) = torch.autograd.grad(y, [x4], gc[None])
    assert torch.equal(dx2, dx)


def test_accuracy_summary_written():
    """max / median of e_hip / e_torch per output over this module's cases (runs after them)"""
    if not RATIOS:
        return
    lines = [f"norm+rope backward {name}: cases {len(r)} max {max(r):.3g} median {float(np.median(r)):.3g}"
             for name, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    path = os.environ.get("VORTA_NORM_ROPE_BWD_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / e_torch over the cases of tests/test_hip_norm_rope_bwd.py (bound: 2)\n" + "\n".join(lines) + "\n")
    assert all(max(r) <= 2.0 for r in RATIOS.values())
