"""GPU: vorta_attn_fwd_varlen (csrc/attn_fwd_varlen.hip) on hand-made tables against float64 attention over exactly the listed
keys, at the bound tests/test_hip_attention.py holds a table launch of the existing kernel to (max |d| <= ATOL_SAME).

Three heads behind the head list (2, 0, 1) with a device count of 2 (the third slot stays untouched), five query groups of 150
positions (the last of 140): with 128-row workgroups a group is a full and a 22-row block, with 256-row ones a block whose last
three waves are idle.  In ONE launch the groups of a slot attend 1, 37 (under a key block), 128 (two whole blocks), 200 (three
blocks and a tail of 8) and 261 = n_kv keys (slot 1: the same lengths rotated).  Every list entry behind a group's length names
row 799 of k and v, which holds NaN: a NaN in the output shows a read past the length."""
import numpy as np
import pytest
import torch

from _util import ATOL_SAME, dev, rounded, to_dev

pytestmark = pytest.mark.gpu

H, S, N_Q, GLEN, N_KV, SENTINEL = 3, 800, 740, 150, 261, 7.0
HEADS, LIVE = [2, 0, 1], 2
LENS = [1, 37, 128, 200, 261]


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    q, k, v = (rng.standard_normal((H, S, 128)) for _ in range(3))
    k[:, S - 1], v[:, S - 1] = np.nan, np.nan
    q_rows = rng.permutation(S - 1)[:N_Q].astype(np.int32)
    n_g = -(-N_Q // GLEN)
    kv_len = np.stack([np.roll(LENS, y) for y in range(H)]).astype(np.int32)
    kv_rows = np.full((H, n_g, N_KV), S - 1, np.int32)
    for y in range(H):
        for g in range(n_g):
            kv_rows[y, g, :kv_len[y, g]] = rng.permutation(S - 1)[:kv_len[y, g]]
    return q, k, v, q_rows, kv_rows, kv_len


def _reference(case, dtype):
    q, k, v, q_rows, kv_rows, kv_len = case
    rq, rk, rv = (rounded(x, dtype) for x in (q, k, v))
    ref = np.full((H, S, 128), SENTINEL)
    for y in range(LIVE):
        h = HEADS[y]
        for g in range(kv_len.shape[1]):
            rows, keys = q_rows[g * GLEN:min((g + 1) * GLEN, N_Q)], kv_rows[y, g, :kv_len[y, g]]
            z = rq[h, rows] @ rk[h, keys].T / np.sqrt(128.0)
            p = np.exp(z - z.max(-1, keepdims=True))
            ref[h, rows] = (p / p.sum(-1, keepdims=True)) @ rv[h, keys]
    return ref


@pytest.mark.parametrize("reverse", [False, True], ids=["index_order", "reversed_order"])
@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_groups_of_different_key_counts_in_one_launch(case, dtype, block_rows, reverse):
    from vorta_amd import ops
    q, k, v, q_rows, kv_rows, kv_len = case
    t = lambda a: torch.as_tensor(a, device=dev())  # noqa: E731
    qd, kd, vd = (to_dev(x, dtype) for x in (q, k, v))
    out = torch.full_like(qd, SENTINEL)
    kv = t(kv_rows)
    n_wg = H * kv_len.shape[1] * -(-GLEN // block_rows)
    order = torch.arange(n_wg - 1, -1, -1, dtype=torch.int32, device=dev()) if reverse else None
    ops.attn_fwd_varlen(qd, kd, vd, out, kv_len=t(kv_len), order=order, n_q=N_Q, q_group_len=GLEN, n_kv=N_KV, q_rows=t(q_rows),
                        kv_rows=kv, kv_rows_stride_g=kv.stride(1), head_list=t(np.array(HEADS, np.int32)), n_heads=H,
                        n_heads_dev=t(np.array([LIVE], np.int32)), block_rows=block_rows)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    assert not np.isnan(got).any(), "a key behind a group's length was read"
    err = np.abs(got - _reference(case, dtype)).max()
    print(f"max |d| {err:.3e} (bound {ATOL_SAME[dtype]})")
    assert err <= ATOL_SAME[dtype]


@pytest.mark.parametrize("family", ["16", "i8"])
def test_refusals_keep_their_code_and_precedence(case, family, monkeypatch):
    """vorta_attn_fwd_varlen and vorta_attn_fwd_varlen_i8 share one entry frame (csrc/attn_common.h fill_var_tables): a wrong
    ext size is VORTA_EINVAL before anything else, split keys are VORTA_EUNSUPPORTED before the tables are looked at, a kv_len
    stride below the groups and a missing kv_rows are VORTA_EINVAL.  Nothing is launched."""
    import ctypes as C
    from vorta_amd import _C, ops
    q, k, v, q_rows, kv_rows, kv_len = case
    t = lambda a: torch.as_tensor(a, device=dev())  # noqa: E731
    qd, kd, vd = (to_dev(np.nan_to_num(x), torch.bfloat16) for x in (q, k, v))
    kv, name, ops_kw = t(kv_rows), "vorta_attn_fwd_varlen", {}
    if family == "i8":
        i8 = ops.i8_quantize_k(qd, kd)
        vd, descale, _ = ops.fp8_quantize_v(vd)
        kd, name, ops_kw = i8.k8, "vorta_attn_fwd_varlen_i8", dict(i8=i8, v_descale=descale)
    kw = dict(kv_len=t(kv_len), n_q=N_Q, q_group_len=GLEN, n_kv=N_KV, q_rows=t(q_rows), kv_rows=kv, kv_rows_stride_g=kv.stride(1),
              **ops_kw)
    out = torch.empty_like(qd)
    einval, eunsupported = f"^{name} failed: VORTA_EINVAL \\(bad argument\\)$", f"^{name} failed: VORTA_EUNSUPPORTED$"
    one_row = dict(kw, kv_len=t(kv_len[:1]).expand(H, -1))  # (slots, groups) with a slot stride of 0 < 5 groups
    with pytest.raises(_C.VortaHipError, match=eunsupported):
        ops.attn_fwd_varlen(qd, kd, vd, out, **kw, n_splits=2)
    with pytest.raises(_C.VortaHipError, match=eunsupported):  # ... before the table checks
        ops.attn_fwd_varlen(qd, kd, vd, out, **one_row, n_splits=2)
    with pytest.raises(ValueError, match=einval):
        ops.attn_fwd_varlen(qd, kd, vd, out, **one_row)
    # a missing kv_rows: the wrapper refuses it by name; behind the wrapper the library answers VORTA_EINVAL
    with pytest.raises(ValueError, match="^kv_len must be int32 \\(slots, groups\\)"):
        ops.attn_fwd_varlen(qd, kd, vd, out, **dict(kw, kv_rows=None))
    a, _ = ops._attn_args(qd, kd, vd, out, **kw)
    a.kv_rows = None
    with pytest.raises(ValueError, match=einval):
        ops._launch_one(a)

    class LongerExt(_C.AttnVarlenExt):  # an ext of another size, as a caller built against another header would pass
        _fields_ = [("more", C.c_int64)]

    monkeypatch.setattr(_C, "AttnVarlenExt", LongerExt)
    for more in ({}, dict(n_splits=2)):  # (... before the parent's checks and the unsupported forms)
        with pytest.raises(ValueError, match=einval):
            ops.attn_fwd_varlen(qd, kd, vd, out, **kw, **more)


def test_split_keys_and_duplicates_are_refused(case):
    from vorta_amd import _C, ops
    q, k, v, q_rows, kv_rows, kv_len = case
    t = lambda a: torch.as_tensor(a, device=dev())  # noqa: E731
    qd, kd, vd = (to_dev(x, torch.bfloat16) for x in (q, k, v))
    kv = t(kv_rows)
    kw = dict(kv_len=t(kv_len), n_q=N_Q, q_group_len=GLEN, n_kv=N_KV, q_rows=t(q_rows), kv_rows=kv, kv_rows_stride_g=kv.stride(1))
    dup = torch.full((N_Q, 1), S - 1, dtype=torch.int32, device=dev())
    for bad in (dict(n_splits=2), dict(dup_rows=dup)):
        with pytest.raises(_C.VortaHipError, match="VORTA_EUNSUPPORTED"):
            ops.attn_fwd_varlen(qd, kd, vd, torch.empty_like(qd), **kw, **bad)
