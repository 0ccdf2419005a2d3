"""CPU-only checks of vorta_qk_norm_rope_bwd and of the differentiable surface built on it: the exported symbol under an
unchanged ABI number, the structure size, argument validation before any launch, the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_abi_and_size():
    from vorta_amd import _C
    lib = _C.lib()
    assert "vorta_qk_norm_rope_bwd" in _C.SYMBOLS and lib.vorta_qk_norm_rope_bwd is not None
    assert lib.vorta_abi_version() == 9 == _C.ABI_VERSION  # a pure addition: the number stays
    assert lib.vorta_sizeof(16) == ctypes.sizeof(_C.NormRopeBwdArgs)
    assert ctypes.sizeof(_C.NormRopeBwdArgs) == 8 + ctypes.sizeof(_C.NormRopeArgs) + 2 * ctypes.sizeof(_C.Tensor) + 24
    assert lib.vorta_sizeof(17) == -1
    header = open(os.path.join(ROOT, "include", "vorta_hip.h")).read()
    assert re.search(r"#define VORTA_NORM_ROPE_BWD_PARTS (\d+)", header).group(1) == str(_C.NORM_ROPE_BWD_PARTS)
    assert "#define VORTA_ABI_VERSION 9" in header and "9 also carries vorta_qk_norm_rope_bwd" in header


def _valid(dweight=True, across=False, heads=24, n_tokens=40):
    """a call that passes validation with fake (never dereferenced on the host) device addresses"""
    from vorta_amd import _C
    a = _C.NormRopeBwdArgs()
    a.struct_size = ctypes.sizeof(_C.NormRopeBwdArgs)
    f = a.fwd
    f.struct_size = ctypes.sizeof(_C.NormRopeArgs)
    f.dtype, f.head_dim, f.heads, f.n_tokens, f.eps, f.across_heads = _C.VORTA_BF16, 128, heads, n_tokens, 1e-6, int(across)
    for t in (f.x, a.g, a.dx):
        t.ptr, t.stride_h, t.stride_s = 0x10000, 128, heads * 128
    f.weight, f.cos, f.sin = 0x20000, 0x30000, 0x40000
    f.rope_tokens = n_tokens
    if dweight:
        a.dweight, a.ws = 0x50000, 0x60000
        a.ws_floats = min((n_tokens + 3) // 4, _C.NORM_ROPE_BWD_PARTS) * (heads * 128 if across else 128)
    return a


def test_refusals_happen_before_any_launch():
    """every case below must come back with its code on a machine without a GPU: nothing may be launched or touched"""
    from vorta_amd import _C
    lib = _C.lib()
    call = lambda a: lib.vorta_qk_norm_rope_bwd(ctypes.byref(a), None)  # noqa: E731
    E, U = _C.VORTA_EINVAL, _C.VORTA_EUNSUPPORTED
    assert lib.vorta_qk_norm_rope_bwd(None, None) == E

    def case(code, edit, **kw):
        a = _valid(**kw)
        edit(a)
        assert call(a) == code, inspect.getsource(edit)

    case(E, lambda a: setattr(a, "struct_size", a.struct_size - 8))
    case(E, lambda a: setattr(a.fwd, "struct_size", 4))
    case(U, lambda a: setattr(a.fwd, "head_dim", 64))
    case(U, lambda a: setattr(a.fwd, "dtype", _C.VORTA_FP32))
    case(U, lambda a: setattr(a.fwd, "heads", 41), across=True)  # more than 10 chunks per lane
    case(E, lambda a: setattr(a.fwd, "heads", 0))
    case(E, lambda a: setattr(a.fwd, "token_offset", -1))
    case(E, lambda a: setattr(a.fwd.x, "ptr", None))
    case(E, lambda a: setattr(a.fwd.x, "ptr", 0x10008))
    case(E, lambda a: setattr(a.g, "ptr", 0x10002))
    case(E, lambda a: setattr(a.g, "stride_s", 24 * 128 + 4))
    case(E, lambda a: setattr(a.dx, "ptr", None))
    case(E, lambda a: setattr(a.dx, "stride_h", 132))
    case(E, lambda a: setattr(a.fwd, "sin", None))  # cos without sin
    case(E, lambda a: setattr(a.fwd, "cos", 0x30004))
    case(E, lambda a: setattr(a.fwd, "weight", 0x20002))
    case(E, lambda a: setattr(a, "ws", None))
    case(E, lambda a: setattr(a, "ws", 0x60004))
    case(E, lambda a: setattr(a, "ws_floats", a.ws_floats - 1))
    case(E, lambda a: setattr(a, "ws_floats", a.ws_floats - 1), across=True, heads=12)
    case(E, lambda a: setattr(a, "ws_floats", 128 * 1023), n_tokens=1 << 20)  # the cap of workgroups is what counts
    # no tokens and no dweight: nothing to do
    a = _valid(dweight=False)
    a.fwd.n_tokens = 0
    assert call(a) == _C.VORTA_OK


def test_missing_symbol_is_a_clear_error(tmp_path, monkeypatch):
    """a library without the new entry point (an older build named by VORTA_HIP_LIB) is refused with a VortaHipError that
    names the symbol, not with an AttributeError at first use"""
    import subprocess
    from vorta_amd import _C
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if __import__("shutil").which(c)), None)
    if cc is None:
        pytest.skip("needs a C compiler")
    src = tmp_path / "old.c"
    names = [n for n in _C.SYMBOLS if n != "vorta_qk_norm_rope_bwd"]
    src.write_text("\n".join(f"int {n}(void) {{ return 9; }}" for n in names) + "\n")
    so = tmp_path / "libold.so"
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    monkeypatch.setattr(_C, "LIB_PATH", str(so))
    monkeypatch.setattr(_C, "_lib", None)
    with pytest.raises(_C.VortaHipError, match="vorta_qk_norm_rope_bwd"):
        _C.lib()


def test_python_surface():
    import torch
    from vorta_amd import ops, routed, torch_ops  # noqa: F401
    from vorta_amd.attention import hunyuan, wan
    from vorta_amd.patch.router import Router
    sig = inspect.signature(ops.qk_norm_rope_bwd).parameters
    for name in ("cos", "sin", "n_tokens", "token_offset", "rope_tokens", "across_heads", "want_dweight"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(routed.qk_norm_rope_autograd)
    assert hasattr(torch.ops.vorta, "qk_norm_rope_grad") and hasattr(torch.ops.vorta, "qk_norm_rope_bwd")
    assert callable(Router.forward_autograd)
    for cls in (hunyuan.HunyuanVideoFlashAttnProcessor, hunyuan.HunyuanVideoFlashAttnProcessorTripleTrain,
                wan.WanAttnProcessor2_0, wan.WanAttnProcessorTripleTrain):
        assert inspect.signature(cls.__init__).parameters["differentiable"].default is False
        assert cls().differentiable is False and cls(differentiable=True).differentiable is True
    for cls in (hunyuan.HunyuanVideoFlashAttnProcessorTripleEval, wan.WanAttnProcessorTripleEval):
        assert cls(differentiable=False).differentiable is False
        with pytest.raises(ValueError, match="top-1"):
            cls(differentiable=True)


def test_router_forward_autograd_on_cpu():
    """the differentiable router is plain torch: it runs and differentiates anywhere"""
    import torch
    from vorta_amd.patch.router import Router
    torch.manual_seed(0)
    r = Router(32, 4).to(torch.bfloat16)
    temb = torch.randn(2, 32).to(torch.bfloat16)
    sc = r.forward_autograd(temb)
    assert sc.shape == (2, 4, 3) and sc.dtype == torch.bfloat16 and sc.requires_grad
    assert torch.allclose(sc.float().sum(-1), torch.ones(2, 4), atol=2e-2)
    (sc * torch.randn(2, 4, 3).to(torch.bfloat16)).sum().backward()
    assert r.linear.weight.grad.abs().sum() > 0 and r.linear.bias.grad.abs().sum() > 0


def test_qk_norm_rope_grad_traces_with_fake_tensors():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vorta_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        x = torch.empty((1, 200, 24 * 128), dtype=torch.bfloat16, device="cuda").unflatten(2, (24, 128)).transpose(1, 2)
        w = torch.empty(128, dtype=torch.bfloat16, device="cuda")
        y = torch.ops.vorta.qk_norm_rope_grad(x, w, 1e-6)
        assert y.shape == x.shape and y.is_contiguous()
        dx, dw = torch.ops.vorta.qk_norm_rope_bwd(x, y, w, 1e-6)
        assert dx.shape == x.shape and dw.shape == (128,) and dw.dtype == torch.float32
