"""CPU-only checks of the backward entry points (ABI 9): exported symbols, structure sizes, argument validation before any
launch, and the compiled kernel's resources (hipcc cross-compiles gfx950 without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_symbols_abi_and_sizes():
    from vorta_amd import _C
    lib = _C.lib()
    for name in ("vorta_attn_bwd", "vorta_mix_experts_bwd", "vorta_cast_grads"):
        assert name in _C.SYMBOLS and getattr(lib, name) is not None
    assert lib.vorta_abi_version() == 9 == _C.ABI_VERSION
    for which, st in ((13, _C.AttnBwdArgs), (14, _C.MixBwdArgs), (15, _C.CastArgs)):
        assert lib.vorta_sizeof(which) == ctypes.sizeof(st)
    assert ctypes.sizeof(_C.AttnBwdArgs) == 8 + ctypes.sizeof(_C.AttnArgs) + 4 * ctypes.sizeof(_C.Tensor) + 16


def _valid_bwd_args():
    """a launch that passes validation with fake (never dereferenced on the host) device addresses"""
    from vorta_amd import _C
    a = _C.AttnBwdArgs()
    a.struct_size = ctypes.sizeof(_C.AttnBwdArgs)
    f = a.fwd
    f.struct_size = ctypes.sizeof(_C.AttnArgs)
    f.dtype, f.head_dim, f.n_heads, f.n_q, f.n_kv, f.n_splits, f.q_valid, f.scale = _C.VORTA_BF16, 128, 1, 64, 64, 1, 64, 0.1
    for t in (f.q, f.k, f.v, f.o, a.d_o, a.dq, a.dk, a.dv):
        t.ptr, t.stride_h, t.stride_s = 0x10000, 64 * 128, 128
    return a


def test_backward_argument_validation_happens_before_any_launch():
    from vorta_amd import _C
    lib = _C.lib()
    call = lambda a: lib.vorta_attn_bwd(ctypes.byref(a), None)  # noqa: E731
    a = _valid_bwd_args()
    a.fwd.n_heads = 0  # a valid block with nothing to do: OK, and nothing is launched
    assert call(a) == _C.VORTA_OK
    a = _valid_bwd_args()
    a.struct_size = 7
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_bwd_args()
    a.dq.ptr = None
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_bwd_args()
    a.fwd.dtype = _C.VORTA_FP8E4M3
    assert call(a) == _C.VORTA_EUNSUPPORTED
    a = _valid_bwd_args()
    a.fwd.head_dim = 64
    assert call(a) == _C.VORTA_EUNSUPPORTED
    a = _valid_bwd_args()
    a.d_o.stride_s = 132  # rows no longer 16-byte aligned
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_bwd_args()
    a.dk.ptr = 0x10004
    assert call(a) == _C.VORTA_EINVAL
    m = _C.MixBwdArgs()
    m.struct_size = ctypes.sizeof(_C.MixBwdArgs)
    m.dtype, m.head_dim, m.heads, m.n_experts, m.n_rows = _C.VORTA_FP32, 128, 1, 3, 8
    assert lib.vorta_mix_experts_bwd(ctypes.byref(m), None) == _C.VORTA_EUNSUPPORTED
    m.dtype = _C.VORTA_BF16  # null tensors
    assert lib.vorta_mix_experts_bwd(ctypes.byref(m), None) == _C.VORTA_EINVAL
    c = _C.CastArgs()
    c.struct_size = ctypes.sizeof(_C.CastArgs)
    c.dtype, c.head_dim, c.heads, c.n_rows, c.n_tensors = _C.VORTA_FP16, 64, 1, 8, 1
    assert lib.vorta_cast_grads(ctypes.byref(c), None) == _C.VORTA_EUNSUPPORTED
    c.head_dim, c.n_tensors = 128, 4
    assert lib.vorta_cast_grads(ctypes.byref(c), None) == _C.VORTA_EINVAL


# what each of the five attention-backward entry points looks at besides q, k, v, o (the statistics pass writes no gradient;
# the two deterministic passes each look at their own buffers only)
_LOOKS_AT = {"vorta_attn_bwd": ("d_o", "dq", "dk", "dv"), "vorta_attn_bwd_stats": ("d_o",),
             "vorta_attn_bwd_kmajor": ("d_o", "dq", "dk", "dv"), "vorta_attn_bwd_dq": ("d_o", "dq"),
             "vorta_attn_bwd_dkv": ("d_o", "dk", "dv")}
_DEFECTS = ("pointer off 16 bytes", "stride_s no multiple", "stride_h no multiple", "stride_s under 128")
# asserted already: here above, in tests/test_host_backward_key_major.py and in tests/test_host_backward_deterministic.py
_ALREADY = {(e, "d_o", "stride_s no multiple") for e in _LOOKS_AT} | {
    ("vorta_attn_bwd", "dk", "pointer off 16 bytes"), ("vorta_attn_bwd_kmajor", "dk", "pointer off 16 bytes"),
    ("vorta_attn_bwd_dq", "dq", "pointer off 16 bytes"), ("vorta_attn_bwd_dkv", "dk", "pointer off 16 bytes"),
    ("vorta_attn_bwd_dkv", "dv", "pointer off 16 bytes")}


@pytest.mark.parametrize("entry,operand,defect", [(e, o, d) for e, ops in _LOOKS_AT.items() for o in ops for d in _DEFECTS
                                                  if (e, o, d) not in _ALREADY])
def test_stride_and_alignment_refusals(entry, operand, defect):
    """d_o (16-bit: 8 elements per 16 bytes) and dq / dk / dv (float: 4) are read and written 16 bytes at a time, 128 channels
    a row: a pointer or a stride that breaks that is refused before any launch (the fake addresses are never dereferenced)"""
    from vorta_amd import _C
    from test_host_backward_key_major import _valid_args
    if entry == "vorta_attn_bwd":
        a = _valid_bwd_args()
        bwd = a
    else:
        a = _valid_args()
        bwd = a.bwd
    t = getattr(bwd, operand)
    per16 = 8 if operand == "d_o" else 4  # elements in 16 bytes
    if defect == "pointer off 16 bytes":
        t.ptr = 0x10000 + 8
    elif defect == "stride_s no multiple":
        t.stride_s = 128 + per16 // 2
    elif defect == "stride_h no multiple":
        t.stride_h = 64 * 128 + per16 // 2
    else:
        t.stride_s = 128 - per16  # (still whole 16-byte units: only the row length is wrong)
    assert getattr(_C.lib(), entry)(ctypes.byref(a), None) == _C.VORTA_EINVAL


def test_python_surface():
    from vorta_amd import ops, routed
    import inspect
    for name in ("attn_bwd", "mix_experts_bwd", "cast_grads"):
        assert callable(getattr(ops, name))
    assert "record" in inspect.signature(routed.routed_attention).parameters
    assert inspect.signature(routed.routed_attention).parameters["record"].default is None
    assert callable(routed.soft_mixture_attention_autograd) and callable(routed.dense_attention_autograd)
    from vorta_amd import torch_ops  # noqa: F401
    import torch
    assert hasattr(torch.ops.vorta, "soft_mixture_attention_grad")


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_backward_kernel_resources():
    """no scratch, no vector-register spill; the LDS images (Q, dO, K, V, P, dS, delta) fit the 160 KiB of a CU"""
    from vorta_amd import build
    res = build.kernel_resources("attn_bwd.hip")
    assert len(res) == 2
    for name, r in res.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 512 and r["lds"] <= 160 * 1024, (name, r)


def test_sources_hold_no_scalar_memory_write():
    """the gradients are written with vector stores and vector float atomics only"""
    words = ["s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic_", "buffer_atomic", "dcache_wb",
                                "dcache_discard")] + ["xnack" + "+", "HSA_" + "XNACK"]
    csrc = os.path.join(ROOT, "vorta_amd", "csrc")
    for fn in ("attn_bwd.hip", "mix.hip"):
        text = open(os.path.join(csrc, fn)).read().lower()
        for w in words:
            assert not re.search(r"\b" + re.escape(w.lower()), text), (fn, w)
