"""CPU-only checks of the deterministic attention backward (vorta_attn_bwd_dq, vorta_attn_bwd_dkv): exported symbols, an
unchanged ABI, argument validation before any launch, the compiled kernels' resources (hipcc cross-compiles gfx950 without a
GPU) and the Python surface of the algorithm switch."""
import ctypes
import os

import pytest

from test_host_backward_key_major import _valid_args

ENTRIES = ("vorta_attn_bwd_dq", "vorta_attn_bwd_dkv")


def test_symbols_and_unchanged_abi():
    from vorta_amd import _C
    lib = _C.lib()
    for name in ENTRIES:
        assert name in _C.SYMBOLS and getattr(lib, name) is not None
    assert lib.vorta_abi_version() == 9 == _C.ABI_VERSION  # a pure addition
    assert lib.vorta_sizeof(17) == -1  # no new struct, no new index
    assert lib.vorta_attn_bwd_kmajor_args_size() == ctypes.sizeof(_C.AttnBwdKmajorArgs)  # both take the existing block
    assert ctypes.sizeof(_C.AttnBwdKmajorArgs) == 8 + ctypes.sizeof(_C.AttnBwdArgs) + 16


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_validation_happens_before_any_launch(entry):
    """(no call below reaches a launch: the fake addresses are never dereferenced)"""
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
    # each entry point requires the buffers it writes and does not look at the others.  (The buffers are looked at for an
    # empty launch too, which is what shows "accepted" here without launching anything.)
    mine, others = (("dq",), ("dk", "dv")) if entry == "vorta_attn_bwd_dq" else (("dk", "dv"), ("dq",))
    for name in mine:
        a = _valid_args()
        getattr(a.bwd, name).ptr = None
        assert call(a) == _C.VORTA_EINVAL
        a = _valid_args()
        getattr(a.bwd, name).ptr = 0x10004  # misaligned
        assert call(a) == _C.VORTA_EINVAL
        a = _valid_args()
        a.bwd.fwd.n_heads = 0
        getattr(a.bwd, name).ptr = None
        assert call(a) == _C.VORTA_EINVAL
    for name in others:
        a = _valid_args()
        a.bwd.fwd.n_heads = 0
        getattr(a.bwd, name).ptr = None
        assert call(a) == _C.VORTA_OK
        a = _valid_args()
        a.bwd.fwd.n_heads = 0
        getattr(a.bwd, name).ptr = 0x10004
        assert call(a) == _C.VORTA_OK


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("source", ["attn_bwd_dq.hip", "attn_bwd_dkv.hip"])
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
    for name in ("attn_bwd_dq", "attn_bwd_dkv"):
        assert callable(getattr(ops, name))
    assert routed.ATTENTION_BACKWARDS == ("query_major", "key_major", "deterministic")
    monkeypatch.setattr(routed, "_attention_backward", None)
    monkeypatch.delenv("VORTA_ATTENTION_BACKWARD", raising=False)
    assert routed.attention_backward() == "query_major"  # still the default
    monkeypatch.setenv("VORTA_ATTENTION_BACKWARD", "deterministic")
    assert routed.attention_backward() == "deterministic"
    assert routed.attention_backward("query_major") == "query_major"  # a call's own choice wins
    monkeypatch.delenv("VORTA_ATTENTION_BACKWARD")
    assert routed.attention_backward("deterministic") == "deterministic"  # the backward= keyword
    vorta_amd.set_attention_backward("deterministic")
    assert routed.attention_backward() == "deterministic"
    routed.set_attention_backward("query_major")
    assert routed.attention_backward() == "query_major"
    for bad in ("Deterministic", "reproducible", "", None):
        with pytest.raises(ValueError):
            routed.set_attention_backward(bad)
    with pytest.raises(ValueError):
        routed.attention_backward("determinstic")
    monkeypatch.setenv("VORTA_ATTENTION_BACKWARD", "fastest")
    monkeypatch.setattr(routed, "_attention_backward", None)
    with pytest.raises(ValueError):
        routed.attention_backward()
    with pytest.raises(ValueError):
        routed._replay_backward([], None, None, None, None, algorithm="fastest")
    routed._replay_backward([], None, None, None, None, algorithm="deterministic")  # (no launch: nothing runs)
