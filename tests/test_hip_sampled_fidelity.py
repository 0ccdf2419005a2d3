"""GPU: vorta_sampled_fidelity (csrc/sampled_fidelity.hip) against the float64 restatement on the same rows
(tests/_sampled_fidelity_restate.py: sums within VORTA_SAMPLED_FIDELITY_CHAIN(n) 2^-24, maxima exact, a row's sum within its
own chain of 11), bf16 and fp16.

Shapes: H in {1, 3}; n in {1, 15, 16, 17, 64, 1025}: fewer rows than the 16 parts, one row short of / exactly / one more than
a row a part, 4 rows a part, and 1025 = 65 rows a part (a lane's fifth visit, a ragged part 15 of 50 rows).  `out` has N > n
rows and the table always names its first and its last row.  Views of `out`: packed (H, N, D), the (N, H D) projection layout,
and offset + padded rows inside a larger storage whose every other element holds a NaN sentinel: a read outside the view
would poison a result, a write would change the sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from _sampled_fidelity_restate import NAMES, check

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
N_ROWS = (1, 15, 16, 17, 64, 1025)
LAYOUTS = ("packed", "projection", "offset_padded")
SENTINEL = 0x7FC1  # a NaN in bf16 and in fp16


def dev():
    return torch.device("cuda:0")


def _place(values: torch.Tensor, layout: str):
    """(view holding `values` (H, N, D), its storage as int16, mask of the storage elements outside the view)"""
    H, N, D = values.shape
    dtype = values.dtype
    if layout == "packed":
        store = torch.full((H, N, D), SENTINEL, dtype=torch.int16, device=dev())
        view = store.view(dtype)
    elif layout == "projection":  # what the attention processors hand over: (N, H D) rows, a head a column block
        store = torch.full((N, H * D), SENTINEL, dtype=torch.int16, device=dev())
        view = store.view(dtype).view(N, H, D).permute(1, 0, 2)
    else:  # rows of 136 elements (272 bytes: 16-byte aligned), the view starts 2 rows and 8 elements into a head's block
        store = torch.full((H, N + 3, D + 8), SENTINEL, dtype=torch.int16, device=dev())
        view = store.view(dtype)[:, 2:2 + N, 8:]
    outside = torch.zeros(store.shape, dtype=torch.bool, device=dev())
    if layout == "offset_padded":
        outside[:] = True
        outside[:, 2:2 + N, 8:] = False
    view.copy_(values)
    assert view.data_ptr() % 16 == 0 and view.stride(2) == 1
    return view, store, outside


def _table(n, N, seed):
    """n distinct rows of [0, N) in random order, the first and the last row of `out` among them (n >= 2)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(N, generator=g)[:n]
    if n >= 2:
        rest = [r for r in rows.tolist() if r not in (0, N - 1)]
        rows = torch.tensor(([0, N - 1] + rest)[:n])[torch.randperm(n, generator=g)]
    return rows.to(torch.int32).to(dev())


def _case(H, n, dtype, seed, N=None, noise=0.05):
    N = N or n + 23
    g = torch.Generator().manual_seed(seed)
    out = torch.randn((H, N, 128), generator=g).to(dtype).to(dev())
    rows = _table(n, N, seed)
    ref = (out[:, rows.long()].float().cpu() + noise * torch.randn((H, n, 128), generator=g)).to(dtype).to(dev())
    return ref, out, rows


@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_against_float64_over_shapes_and_views(dtype, n):
    from vorta_amd import ops
    for H in (1, 3):
        ref, out, rows = _case(H, n, DTYPES[dtype], seed=100 * H + n)
        if n >= 2:
            assert 0 in rows.tolist() and out.shape[1] - 1 in rows.tolist()
        for layout in LAYOUTS:
            view, store, outside = _place(out, layout)
            for row_errors in (False, True):
                fid = ops.sampled_fidelity(ref, view, rows, row_errors=row_errors)
                torch.cuda.synchronize()
                case = f"{dtype} H {H} n {n} {layout}{' rows' if row_errors else ''}"
                check(fid, ref, out, rows, case=case)
                assert (fid.row_sq_err is not None) == row_errors
                assert bool((store[outside] == SENTINEL).all()), (case, "storage outside the view changed")
                assert torch.equal(view, out), (case, "the output changed")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_head_lists_with_device_counts_and_prefill(dtype):
    """head lists as the attention launches take them: host counts and device counts of 0, some and all of the slots;
    heads the launch does not name, and slots at or past the device count, keep the caller's prefill bit for bit"""
    from vorta_amd import ops
    H, n = 3, 17
    ref, out, rows = _case(H, n, DTYPES[dtype], seed=31)
    lst = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev())

    def prefilled():
        f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=dev())  # noqa: E731
        return ops.SampledFidelity(f(H), f(H), f(H), f(H), f(H), f(H, n), n * 128, rows)

    for count in (0, 1, 2, 3):
        heads = lst[:count].tolist()
        cnt = torch.tensor([count], dtype=torch.int32, device=dev())
        by_dev = ops.sampled_fidelity(ref, out, rows, head_list=lst, n_heads=H, n_heads_dev=cnt, row_errors=True, into=prefilled())
        check(by_dev, ref, out, rows, heads=heads, case=f"{dtype} device count {count}", prefill=7.0)
        by_host = ops.sampled_fidelity(ref, out, rows, head_list=lst, n_heads=count, row_errors=True, into=prefilled())
        for name in NAMES + ("row_sq_err",):
            assert torch.equal(getattr(by_dev, name), getattr(by_host, name)), (count, name)
        fresh = ops.sampled_fidelity(ref, out, rows, head_list=lst, n_heads=count)
        check(fresh, ref, out, rows, heads=heads, case=f"{dtype} host count {count}")  # unmeasured: NaN
    # two launches into one record, as routed_attention files the coreset and the sliding heads
    both = ops.sampled_fidelity(ref, out, rows, head_list=lst[:1], n_heads=1)
    both = ops.sampled_fidelity(ref, out, rows, head_list=lst[2:], n_heads=1, into=both)
    check(both, ref, out, rows, heads=[2, 1], case=f"{dtype} two lists")
    # no head list: slot = head
    part = ops.sampled_fidelity(ref, out, rows, n_heads=2)
    check(part, ref, out, rows, heads=[0, 1], case=f"{dtype} first two heads")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_zero_rows_identical_rows_and_zero_reference(dtype):
    from vorta_amd import ops
    dt = DTYPES[dtype]
    out = torch.randn((3, 9, 128), device=dev()).to(dt)
    none = torch.empty((0,), dtype=torch.int32, device=dev())
    fid = ops.sampled_fidelity(out[:, :0], out, none, head_list=torch.tensor([1], dtype=torch.int32, device=dev()))
    for name in NAMES:  # zeros for the listed head, NaN elsewhere
        got = getattr(fid, name)
        assert got[1] == 0 and bool(torch.isnan(got[[0, 2]]).all()), name
    assert fid.rel_error()[1] == 0
    ref, out, rows = _case(3, 64, dt, seed=5)
    same = ops.sampled_fidelity(out[:, rows.long()].contiguous(), out, rows, row_errors=True)
    assert (same.sq_err == 0).all() and (same.max_err == 0).all() and (same.row_sq_err == 0).all()
    assert (same.rel_error() == 0).all() and (same.psnr() == float("inf")).all()
    zero = ops.sampled_fidelity(torch.zeros_like(ref), out, rows)
    check(zero, torch.zeros_like(ref), out, rows, case=f"{dtype} zero reference")
    assert (zero.sq_ref == 0).all() and (zero.rel_error() == float("inf")).all()
    with pytest.raises(ValueError):
        ops.sampled_fidelity(ref, out, rows[:-1])
    with pytest.raises(ValueError):
        ops.sampled_fidelity(ref, out.float(), rows)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nan_and_inf_reach_their_head_and_statistic_only(dtype):
    from vorta_amd import ops
    dt = DTYPES[dtype]
    H, n = 3, 1025
    ref, out, rows = _case(H, n, dt, seed=11)
    clean = ops.sampled_fidelity(ref, out, rows, row_errors=True)
    last = int(rows[n - 1])
    o2, r2 = out.clone(), ref.clone()
    o2[1, last, 127] = float("nan")      # head 1: the output, the last element of the last sample position
    r2[2, 17, 3] = float("inf")          # head 2: the reference
    o2[0, [r for r in range(out.shape[1]) if r not in rows.tolist()][0], 5] = float("nan")  # a row the table does not name
    fid = ops.sampled_fidelity(r2, o2, rows, row_errors=True)
    check(fid, r2, o2, rows, case=f"{dtype} NaN and Inf")
    for name in NAMES + ("row_sq_err",):
        assert torch.equal(getattr(fid, name)[0], getattr(clean, name)[0]), name  # head 0: the bits of the clean run
    assert torch.isnan(fid.sq_err[1]) and torch.isnan(fid.max_err[1]) and torch.isnan(fid.row_sq_err[1, n - 1])
    assert fid.sq_ref[1] == clean.sq_ref[1] and fid.max_ref[1] == clean.max_ref[1] and fid.range_ref[1] == clean.range_ref[1]
    assert torch.equal(fid.row_sq_err[1, :n - 1], clean.row_sq_err[1, :n - 1])
    inf = float("inf")
    assert fid.sq_ref[2] == inf and fid.max_ref[2] == inf and fid.range_ref[2] == inf and fid.sq_err[2] == inf and fid.max_err[2] == inf
    o2[2, int(rows[17]), 3] = inf        # inf meets inf: NaN in the error, the reference's own statistics stay inf
    fid = ops.sampled_fidelity(r2, o2, rows)
    check(fid, r2, o2, rows, case=f"{dtype} Inf meets Inf")
    assert torch.isnan(fid.sq_err[2]) and torch.isnan(fid.max_err[2]) and fid.sq_ref[2] == inf
    r3 = ref.clone()
    r3[0, 0, 0] = float("nan")           # a NaN in the reference: every statistic of that head
    fid = ops.sampled_fidelity(r3, out, rows)
    check(fid, r3, out, rows, case=f"{dtype} NaN in the reference")
    assert all(bool(torch.isnan(getattr(fid, name)[0])) for name in NAMES)
    assert all(bool(torch.isfinite(getattr(fid, name)[1:]).all()) for name in NAMES)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_five_runs_on_two_streams_give_equal_bits(dtype):
    from vorta_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.vorta.*)
    ref, out, rows = _case(3, 1025, DTYPES[dtype], seed=17)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())]
    runs = []
    for i in range(5):
        with torch.cuda.stream(streams[i % 2]):
            runs.append(ops.sampled_fidelity(ref, out, rows, row_errors=True))
    torch.cuda.synchronize()
    runs.append(ops.sampled_fidelity(ref, out, rows, row_errors=True))  # and the default stream
    torch.cuda.synchronize()
    for r in runs[1:]:
        for name in NAMES + ("row_sq_err",):
            assert torch.equal(getattr(r, name), getattr(runs[0], name)), name
    got = torch.ops.vorta.sampled_fidelity(ref, out, rows, None, -1, None, True)  # the registered operator: the same launcher
    for t, name in zip(got, ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref", "row_sq_err")):
        assert torch.equal(t, getattr(runs[0], name)), name


def test_error_codes_with_nothing_launched():
    """every documented bad argument returns its code before anything is launched: the outputs keep their prefill"""
    from vorta_amd import _C
    H, n, N = 2, 16, 20
    ref = torch.randn((H, n, 128), device=dev()).half()
    out = torch.randn((H, N, 128), device=dev()).half()
    rows = torch.arange(n, dtype=torch.int32, device=dev())
    stats = torch.full((5, H), 7.0, dtype=torch.float32, device=dev())
    rowsum = torch.full((H, n), 7.0, dtype=torch.float32, device=dev())
    ws = torch.full((H * _C.SAMPLED_FIDELITY_PARTS * _C.SAMPLED_FIDELITY_WS_FLOATS + 4,), 7.0, dtype=torch.float32, device=dev())
    lst = torch.arange(H + 1, dtype=torch.int32, device=dev())
    lib = _C.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def args(**over):
        a = _C.SampledFidelityArgs()
        a.struct_size = C.sizeof(_C.SampledFidelityArgs)
        a.dtype, a.head_dim, a.n_heads, a.n_rows = _C.VORTA_FP16, 128, H, n
        a.ref = _C.Tensor(ref.data_ptr(), ref.stride(0), ref.stride(1))
        a.out = _C.Tensor(out.data_ptr(), out.stride(0), out.stride(1))
        a.rows = rows.data_ptr()
        a.sq_ref, a.max_ref, a.sq_err, a.max_err, a.range_ref = (stats[i].data_ptr() for i in range(5))
        a.row_sq_err, a.ws = rowsum.data_ptr(), ws.data_ptr()
        for key, val in over.items():
            setattr(a, key, val)
        return a

    EINVAL, EUNSUP = _C.VORTA_EINVAL, _C.VORTA_EUNSUPPORTED
    odd = lambda t: _C.Tensor(t.data_ptr() + 2, t.stride(0), t.stride(1))  # noqa: E731
    bad = [("struct_size", dict(struct_size=8), EINVAL), ("dtype fp32", dict(dtype=_C.VORTA_FP32), EUNSUP),
           ("dtype int8", dict(dtype=_C.VORTA_INT8), EUNSUP), ("head_dim 64", dict(head_dim=64), EUNSUP),
           ("negative heads", dict(n_heads=-1), EINVAL), ("negative rows", dict(n_rows=-1), EINVAL),
           ("null sq_ref", dict(sq_ref=None), EINVAL), ("null max_ref", dict(max_ref=None), EINVAL),
           ("null sq_err", dict(sq_err=None), EINVAL), ("null max_err", dict(max_err=None), EINVAL),
           ("misaligned sq_err", dict(sq_err=stats[2].data_ptr() + 2), EINVAL),
           ("misaligned range_ref", dict(range_ref=stats[4].data_ptr() + 1), EINVAL),
           ("misaligned row_sq_err", dict(row_sq_err=rowsum.data_ptr() + 2), EINVAL),
           ("null rows", dict(rows=None), EINVAL), ("misaligned rows", dict(rows=rows.data_ptr() + 2), EINVAL),
           ("misaligned head_list", dict(head_list=lst.data_ptr() + 2), EINVAL),
           ("misaligned n_heads_dev", dict(n_heads_dev=lst.data_ptr() + 1), EINVAL),
           ("null ws", dict(ws=None), EINVAL), ("misaligned ws", dict(ws=ws.data_ptr() + 4), EINVAL),
           ("null ref", dict(ref=_C.Tensor(None, ref.stride(0), ref.stride(1))), EINVAL),
           ("null out", dict(out=_C.Tensor(None, out.stride(0), out.stride(1))), EINVAL),
           ("misaligned ref", dict(ref=odd(ref)), EINVAL), ("misaligned out", dict(out=odd(out)), EINVAL),
           ("odd row stride", dict(out=_C.Tensor(out.data_ptr(), out.stride(0), 129)), EINVAL),
           ("odd head stride", dict(ref=_C.Tensor(ref.data_ptr(), n * 128 + 4, 128)), EINVAL)]
    for what, over, code in bad:
        assert lib.vorta_sampled_fidelity(C.byref(args(**over)), stream) == code, what
    assert lib.vorta_sampled_fidelity(None, stream) == EINVAL
    # bad arguments are reported even when there is no head to launch for; no heads alone is fine and launches nothing
    assert lib.vorta_sampled_fidelity(C.byref(args(n_heads=0, ws=None)), stream) == EINVAL
    assert lib.vorta_sampled_fidelity(C.byref(args(n_heads=0)), stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert (stats == 7.0).all() and (rowsum == 7.0).all() and (ws == 7.0).all()
    # and the good call writes: null tensors and a null table pass with no rows
    assert lib.vorta_sampled_fidelity(C.byref(args(n_rows=0, rows=None, ref=_C.Tensor(None, 0, 128), out=_C.Tensor(None, 0, 128))),
                                      stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert (stats == 0.0).all() and (rowsum == 7.0).all()
    assert lib.vorta_sampled_fidelity(C.byref(args()), stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert (stats[0] > 0).all() and (rowsum != 7.0).all()
    assert np.isfinite(stats.cpu().numpy()).all()


def test_into_without_a_range():
    """an `into` built without `range_ref` (the NamedTuple's default): the library takes NULL there; the other four statistics
    are those of a fresh record, bit for bit"""
    from vorta_amd import ops
    ref, out, rows = _case(3, 17, torch.bfloat16, seed=9)
    fresh = ops.sampled_fidelity(ref, out, rows)
    nan = lambda: torch.full((3,), float("nan"), dtype=torch.float32, device=dev())  # noqa: E731
    bare = ops.SampledFidelity(nan(), nan(), nan(), nan(), n=17 * 128, rows=rows)
    got = ops.sampled_fidelity(ref, out, rows, into=bare)
    torch.cuda.synchronize()
    assert got.range_ref is None
    for name in ("sq_ref", "max_ref", "sq_err", "max_err"):
        assert torch.equal(getattr(got, name), getattr(fresh, name)), name
    with pytest.raises(ValueError, match="range_ref"):
        got.psnr(over="range")
