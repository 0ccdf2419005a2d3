"""CPU-only checks of the key-major attention backward (vorta_attn_bwd_stats, vorta_attn_bwd_kmajor): exported symbols, the
new argument block's size, argument validation before any launch, the compiled kernels' resources (hipcc cross-compiles
gfx950 without a GPU) and the Python surface of the algorithm switch."""
import ctypes
import inspect
import os

import pytest


def test_symbols_abi_and_sizes():
    from vorta_amd import _C
    lib = _C.lib()
    for name in ("vorta_attn_bwd_stats", "vorta_attn_bwd_kmajor", "vorta_attn_bwd_kmajor_args_size"):
        assert name in _C.SYMBOLS and getattr(lib, name) is not None
    assert lib.vorta_abi_version() == 9 == _C.ABI_VERSION  # a pure addition
    assert lib.vorta_attn_bwd_kmajor_args_size() == ctypes.sizeof(_C.AttnBwdKmajorArgs)
    assert ctypes.sizeof(_C.AttnBwdKmajorArgs) == 8 + ctypes.sizeof(_C.AttnBwdArgs) + 16
    assert lib.vorta_sizeof(13) == ctypes.sizeof(_C.AttnBwdArgs) and lib.vorta_sizeof(17) == -1  # the old indices stay


def _valid_args():
    """a launch that passes validation with fake (never dereferenced on the host) device addresses"""
    from vorta_amd import _C
    a = _C.AttnBwdKmajorArgs()
    a.struct_size = ctypes.sizeof(_C.AttnBwdKmajorArgs)
    a.stats, a.stats_stride_h = 0x20000, 2 * 64
    b = a.bwd
    b.struct_size = ctypes.sizeof(_C.AttnBwdArgs)
    f = b.fwd
    f.struct_size = ctypes.sizeof(_C.AttnArgs)
    f.dtype, f.head_dim, f.n_heads, f.n_q, f.n_kv, f.n_splits, f.q_valid, f.scale = _C.VORTA_BF16, 128, 1, 64, 64, 1, 64, 0.1
    for t in (f.q, f.k, f.v, f.o, b.d_o, b.dq, b.dk, b.dv):
        t.ptr, t.stride_h, t.stride_s = 0x10000, 64 * 128, 128
    return a


@pytest.mark.parametrize("entry", ["vorta_attn_bwd_stats", "vorta_attn_bwd_kmajor"])
def test_argument_validation_happens_before_any_launch(entry):
    from vorta_amd import _C
    fn = getattr(_C.lib(), entry)
    call = lambda a: fn(ctypes.byref(a), None)  # noqa: E731
    a = _valid_args()
    a.bwd.fwd.n_heads = 0  # a valid block with nothing to do: OK, and nothing is launched
    assert call(a) == _C.VORTA_OK
    a = _valid_args()
    a.struct_size = 7
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_args()
    a.bwd.struct_size = 7
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_args()
    a.stats = None
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_args()
    a.stats_stride_h = 2 * 64 - 2  # does not hold two floats per position
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_args()
    a.bwd.d_o.stride_s = 132  # rows no longer 16-byte aligned
    assert call(a) == _C.VORTA_EINVAL
    a = _valid_args()
    a.bwd.fwd.dtype = _C.VORTA_FP8E4M3
    assert call(a) == _C.VORTA_EUNSUPPORTED
    a = _valid_args()
    a.bwd.fwd.head_dim = 64
    assert call(a) == _C.VORTA_EUNSUPPORTED
    a = _valid_args()
    a.bwd.fwd.q_block_table, a.bwd.fwd.n_q_blocks, a.bwd.fwd.block_rows = 0x30000, 1, 128  # a table without n_key_lists
    assert call(a) == _C.VORTA_EINVAL
    if entry == "vorta_attn_bwd_kmajor":  # (the statistics pass writes no gradient and does not look at the three buffers)
        a = _valid_args()
        a.bwd.dq.ptr = None
        assert call(a) == _C.VORTA_EINVAL
        a = _valid_args()
        a.bwd.dk.ptr = 0x10004
        assert call(a) == _C.VORTA_EINVAL


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("source", ["attn_bwd_stats.hip", "attn_bwd_kmajor.hip"])
def test_kernel_resources(source):
    """no scratch, no vector-register spill, at most the 512 registers of one wave per SIMD, LDS within the 160 KiB of a CU"""
    from vorta_amd import build
    assert source in build.SOURCES
    res = build.kernel_resources(source)
    assert len(res) == 2  # bf16 and fp16
    for name, r in res.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 512 and r["lds"] <= 160 * 1024, (name, r)


def test_python_surface(monkeypatch):
    import vorta_amd
    from vorta_amd import ops, routed
    for name in ("attn_bwd_stats", "attn_bwd_key_major", "attn_bwd_stats_shape"):
        assert callable(getattr(ops, name))
    assert ops.attn_bwd_stats_shape(3, 70) == (3, 70, 2)
    for fn in (routed.soft_mixture_attention_autograd, routed.dense_attention_autograd):
        assert inspect.signature(fn).parameters["backward"].default is None
    assert inspect.signature(routed._replay_backward).parameters["algorithm"].default == "query_major"
    monkeypatch.setattr(routed, "_attention_backward", None)
    monkeypatch.delenv("VORTA_ATTENTION_BACKWARD", raising=False)
    assert routed.attention_backward() == "query_major"  # the default
    monkeypatch.setenv("VORTA_ATTENTION_BACKWARD", "key_major")
    assert routed.attention_backward() == "key_major"
    assert routed.attention_backward("query_major") == "query_major"  # a call's own choice wins
    monkeypatch.setenv("VORTA_ATTENTION_BACKWARD", "fastest")
    with pytest.raises(ValueError):
        routed.attention_backward()
    monkeypatch.delenv("VORTA_ATTENTION_BACKWARD")
    vorta_amd.set_attention_backward("key_major")
    assert routed.attention_backward() == "key_major"
    routed.set_attention_backward("query_major")
    assert routed.attention_backward() == "query_major"
    for bad in ("fastest", "", None):
        with pytest.raises(ValueError):
            routed.set_attention_backward(bad)
    with pytest.raises(ValueError):
        routed.attention_backward("keymajor")
    with pytest.raises(ValueError):
        routed._replay_backward([], None, None, None, None, algorithm="fastest")
