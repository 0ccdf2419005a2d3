"""GPU: vorta_expert_fidelity (csrc/expert_fidelity.hip) against float64 numpy, bf16 and fp16.

Bound on the sums (not fitted): the header states the longest chain of float32 roundings a sum passes through,
VORTA_FIDELITY_CHAIN(n_rows) = ceil(ceil(n_rows / 64) / 16) + 21; every term of a sum is a square, so
|sum - exact| <= CHAIN 2^-24 exact.  The bound itself must be under 1e-4 at every shape here (and at Hunyuan-129f: 138 2^-24).
Maxima are exact: the float32 rounding of a difference is monotone, so max |fl(d)| = fl(max |d|), the float64 maximum rounded
once.  Non-finite results must be the float64 evaluation's (NaN where it has NaN, inf where it has inf), head by head.

Shapes: H in {1, 3}; n_rows in {1, 7, 64, 65, 1000, 1025}: fewer rows than the 64 parts, one row a part, a ragged last range
(1000 = 62 x 16 + 8, part 63 empty) and 1025 = 16 rows a workgroup pass x 64 parts + 1 (17 rows a part: a lane's second visit,
a ragged part 60, parts 61-63 empty).  Views: packed, head-permuted ((N, H, D) storage), and offset + padded rows inside a
larger storage whose every other element holds a NaN sentinel: a read outside the views would poison a result, a write would
change the sentinel.  VORTA_EXPERT_FIDELITY_ACCURACY_OUT names a file that receives the largest observed error over bound
(profiles/expert_fidelity_accuracy.txt is such a file)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
N_ROWS = (1, 7, 64, 65, 1000, 1025)
LAYOUTS = ("packed", "permuted", "offset_padded")
SENTINEL = 0x7FC1  # a NaN in bf16 and in fp16
RATIOS = {}  # case -> largest |sum - exact| / (CHAIN 2^-24 exact) seen


def dev():
    return torch.device("cuda:0")


def chain(n_rows):
    from vorta_amd import _C
    return _C.fidelity_chain(n_rows)


def _place(values: torch.Tensor, layout: str):
    """(view holding `values` (H, N, D), its storage as int16, mask of the storage elements outside the view)"""
    H, N, D = values.shape
    dtype = values.dtype
    if layout == "packed":
        store = torch.full((H, N, D), SENTINEL, dtype=torch.int16, device=dev())
        view = store.view(dtype)
    elif layout == "permuted":
        store = torch.full((N, H, D), SENTINEL, dtype=torch.int16, device=dev())
        view = store.view(dtype).permute(1, 0, 2)
    else:  # rows of 136 elements (272 bytes: 16-byte aligned), the view starts 2 rows and 8 elements into a head's block
        store = torch.full((H, N + 3, D + 8), SENTINEL, dtype=torch.int16, device=dev())
        view = store.view(dtype)[:, 2:2 + N, 8:]
    outside = torch.ones(store.shape, dtype=torch.bool, device=dev())
    if layout == "packed":
        outside[:] = False
    elif layout == "permuted":
        outside[:] = False
    else:
        outside[:, 2:2 + N, 8:] = False
    view.copy_(values)
    assert view.data_ptr() % 16 == 0 and view.stride(2) == 1
    return view, store, outside


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def reference(xs, mixed):
    """float64 numpy: sq_ref, max_ref, range_ref (H,), sq_err, max_err (H, 3) with NaN in the mixed column when not given"""
    x0 = _f64(xs[0])
    H = x0.shape[0]
    flat = x0.reshape(H, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        sq_ref = (flat * flat).sum(1)
        if flat.shape[1]:
            max_ref, range_ref = np.abs(flat).max(1), flat.max(1) - flat.min(1)
        else:
            max_ref, range_ref = np.zeros(H), np.zeros(H)
        sq_err, max_err = np.full((H, 3), np.nan), np.full((H, 3), np.nan)
        for j, t in enumerate((xs[1], xs[2], mixed)):
            if t is None:
                continue
            d = (_f64(t) - x0).reshape(H, -1)
            sq_err[:, j] = (d * d).sum(1)
            max_err[:, j] = np.abs(d).max(1) if d.shape[1] else 0.0
    return dict(sq_ref=sq_ref, max_ref=max_ref, range_ref=range_ref, sq_err=sq_err, max_err=max_err)


def check(fid, ref, n_rows, case):
    """sums within CHAIN 2^-24 (relative; exact zeros and non-finite values as the reference has them), maxima exact"""
    bound = chain(n_rows) * U
    assert bound < 1e-4, (n_rows, bound)
    worst = 0.0
    for name in ("sq_ref", "sq_err"):
        got, want = getattr(fid, name).double().cpu().numpy(), ref[name]
        assert got.shape == want.shape
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (case, name, got, want)
        zero = fin & (want == 0)
        assert (got[zero] == 0).all(), (case, name)
        pos = fin & (want > 0)
        ratio = np.abs(got[pos] - want[pos]) / (bound * want[pos])
        if ratio.size:
            worst = max(worst, float(ratio.max()))
        print(f"{case} {name}: n_rows {n_rows} chain {chain(n_rows)} bound {bound:.3e} largest error / bound "
              f"{float(ratio.max()) if ratio.size else 0.0:.4f}")
    RATIOS[case] = max(RATIOS.get(case, 0.0), worst)
    assert worst <= 1.0, (case, worst)
    with np.errstate(over="ignore"):
        for name in ("max_ref", "max_err", "range_ref"):
            got, want = getattr(fid, name).cpu().numpy(), ref[name].astype(np.float32)  # one rounding of the exact value
            assert np.array_equal(got, want, equal_nan=True), (case, name, got, want)
    assert fid.n == n_rows * 128


def _random_case(H, N, dtype, seed, mixed=True, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn((H, N, 128), generator=g) * scale
    x1 = x0 + 0.05 * scale * torch.randn((H, N, 128), generator=g)
    x2 = x0 + 0.5 * scale * torch.randn((H, N, 128), generator=g)
    m = 0.2 * x0 + 0.5 * x1 + 0.3 * x2
    return [t.to(dtype).to(dev()) for t in ((x0, x1, x2, m) if mixed else (x0, x1, x2))]


@pytest.mark.parametrize("n_rows", N_ROWS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_against_float64_over_shapes_and_views(dtype, n_rows):
    from vorta_amd import ops
    for H in (1, 3):
        for layout in LAYOUTS:
            for mixed in (True, False):
                vals = _random_case(H, n_rows, DTYPES[dtype], seed=1000 * H + n_rows, mixed=mixed)
                placed = [_place(v, layout) for v in vals]
                views = [p[0] for p in placed]
                fid = ops.expert_fidelity(views[:3], views[3] if mixed else None)
                torch.cuda.synchronize()
                case = f"{dtype} H {H} {layout} {'mixed' if mixed else 'no mixed'}"
                check(fid, reference(vals[:3], vals[3] if mixed else None), n_rows, case)
                assert bool(torch.isnan(fid.sq_err[:, 2]).all()) == (not mixed)  # written only when `mixed` is given
                for (view, store, outside), v in zip(placed, vals):
                    assert bool((store[outside] == SENTINEL).all()), (case, "storage outside a view changed")
                    assert torch.equal(view, v), (case, "an input changed")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_zero_rows_and_zero_heads(dtype):
    from vorta_amd import ops
    dt = DTYPES[dtype]
    x = torch.empty((3, 0, 128), dtype=dt, device=dev())
    for mixed in (None, x):
        fid = ops.expert_fidelity([x, x, x], mixed)
        assert fid.sq_ref.tolist() == [0.0] * 3 and fid.max_ref.tolist() == [0.0] * 3 and fid.range_ref.tolist() == [0.0] * 3
        cols = 3 if mixed is not None else 2
        assert (fid.sq_err[:, :cols] == 0).all() and (fid.max_err[:, :cols] == 0).all()
        assert fid.rel_error()[:, :cols].tolist() == [[0.0] * cols] * 3
    y = torch.empty((0, 5, 128), dtype=dt, device=dev())
    fid = ops.expert_fidelity([y, y, y], y)
    assert fid.sq_ref.shape == (0,) and fid.sq_err.shape == (0, 3)
    with pytest.raises(ValueError):
        ops.expert_fidelity([x, x], None)
    with pytest.raises(ValueError):
        ops.expert_fidelity([x, x, x.float()], None)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_identical_buffers_give_exact_zeros_and_zero_reference_gives_inf(dtype):
    from vorta_amd import ops
    dt = DTYPES[dtype]
    x0, x1, x2, m = _random_case(3, 65, dt, seed=5)
    fid = ops.expert_fidelity([x0, x0.clone(), x0.clone()], x0.clone())
    assert (fid.sq_err == 0).all() and (fid.max_err == 0).all() and (fid.rel_error() == 0).all()
    assert (fid.psnr() == float("inf")).all()
    check(fid, reference([x0, x0, x0], x0), 65, f"{dtype} identical")
    z = torch.zeros_like(x0)
    fid = ops.expert_fidelity([z, x1, z.clone()], m)
    check(fid, reference([z, x1, z], m), 65, f"{dtype} zero reference")
    assert (fid.sq_ref == 0).all() and (fid.max_ref == 0).all()
    rel = fid.rel_error()
    assert (rel[:, 0] == float("inf")).all() and (rel[:, 1] == 0).all() and (rel[:, 2] == float("inf")).all()


def test_fp16_extremes_and_subnormals():
    """entries at +-65504 (differences of 131 008: squares of 1.7e10, nothing overflows in float32) and fp16 subnormals
    (multiples of 2^-24: their differences and squares are normal float32 numbers)"""
    from vorta_amd import ops
    H, N = 3, 65
    g = torch.Generator().manual_seed(9)
    x0, x1, x2, m = (t.cpu() for t in _random_case(H, N, torch.float16, seed=9))
    big = torch.randint(0, 2, (H, N, 128), generator=g).bool()
    x0 = torch.where(big, torch.tensor(65504.0, dtype=torch.float16), torch.tensor(-65504.0, dtype=torch.float16))
    x1 = -x0  # every difference is +-131 008
    sub = (torch.randint(-1023, 1024, (H, N, 128), generator=g).float() * 2.0 ** -24).half()  # subnormals, both signs, zeros
    assert bool((sub.abs() < 2.0 ** -14).all()) and bool((sub != 0).any())
    xs = [t.to(dev()) for t in (x0, x1, x2, m)]
    fid = ops.expert_fidelity(xs[:3], xs[3])
    check(fid, reference(xs[:3], xs[3]), N, "fp16 +-65504")
    assert (fid.max_ref == 65504.0).all() and (fid.max_err[:, 0] == 131008.0).all() and (fid.range_ref == 131008.0).all()
    ys = [sub.to(dev()), (sub * 3).to(dev()), torch.zeros_like(sub).to(dev()), (-sub).to(dev())]
    fid = ops.expert_fidelity(ys[:3], ys[3])
    check(fid, reference(ys[:3], ys[3]), N, "fp16 subnormals")
    assert (fid.sq_ref > 0).all() and (fid.max_ref < 2.0 ** -14).all()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nan_and_inf_reach_their_head_only(dtype):
    from vorta_amd import ops
    dt = DTYPES[dtype]
    H, N = 3, 1000
    clean = _random_case(H, N, dt, seed=11)
    want_clean = ops.expert_fidelity(clean[:3], clean[3])
    xs = [t.clone() for t in clean]
    xs[1][1, 999, 127] = float("nan")   # head 1, the coreset expert: the last element of the ragged last range
    xs[0][2, 17, 3] = float("inf")      # head 2, the full expert: every column of head 2 sees it
    fid = ops.expert_fidelity(xs[:3], xs[3])
    ref = reference(xs[:3], xs[3])
    check(fid, ref, N, f"{dtype} NaN and Inf")
    nan, inf = float("nan"), float("inf")
    # head 0: the bits of the clean run
    for name in ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err"):
        assert torch.equal(getattr(fid, name)[0], getattr(want_clean, name)[0]), name
    # head 1: the coreset column is NaN (sum and maximum), nothing else
    assert torch.isnan(fid.sq_err[1, 0]) and torch.isnan(fid.max_err[1, 0])
    assert torch.equal(fid.sq_err[1, 1:], want_clean.sq_err[1, 1:]) and torch.equal(fid.max_err[1, 1:], want_clean.max_err[1, 1:])
    assert fid.sq_ref[1] == want_clean.sq_ref[1] and fid.max_ref[1] == want_clean.max_ref[1]
    # head 2: an infinite reference, infinitely far from every finite expert
    assert fid.sq_ref[2] == inf and fid.max_ref[2] == inf and fid.range_ref[2] == inf
    assert (fid.sq_err[2] == inf).all() and (fid.max_err[2] == inf).all()
    # inf - inf is NaN: where the mixed output is infinite at the same place, its column is NaN
    xs[3][2, 17, 3] = inf
    fid = ops.expert_fidelity(xs[:3], xs[3])
    check(fid, reference(xs[:3], xs[3]), N, f"{dtype} Inf meets Inf")
    assert torch.isnan(fid.sq_err[2, 2]) and torch.isnan(fid.max_err[2, 2]) and fid.sq_err[2, 0] == inf
    # a NaN in the full expert: every statistic of that head, the maxima and the range included
    xs = [t.clone() for t in clean]
    xs[0][0, 0, 0] = nan
    fid = ops.expert_fidelity(xs[:3], xs[3])
    check(fid, reference(xs[:3], xs[3]), N, f"{dtype} NaN in the reference")
    assert all(bool(torch.isnan(getattr(fid, n)[0]).all()) for n in ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err"))
    assert all(bool(torch.isfinite(getattr(fid, n)[1:]).all()) for n in ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err"))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_huge_outlier_in_the_last_row_of_the_last_range(dtype):
    """1025 rows: 17 a part, the last non-empty part (60) holds rows 1020 .. 1024; the outlier sits in row 1024.  bf16: 2^60
    (its square, 2^120, is a float32 number; the difference against values near 1 is rounded, which the chain counts);
    fp16: 60 000."""
    from vorta_amd import ops
    dt = DTYPES[dtype]
    big = 2.0 ** 60 if dtype == "bf16" else 60000.0
    for where in (0, 1, 3):  # in the full expert, in the coreset expert, in the mixed output
        xs = _random_case(3, 1025, dt, seed=13 + where)
        xs[where][2, 1024, 127] = big
        fid = ops.expert_fidelity(xs[:3], xs[3])
        check(fid, reference(xs[:3], xs[3]), 1025, f"{dtype} outlier in tensor {where}")
        if where == 0:
            assert fid.max_ref[2] == big and (fid.max_err[2] >= big / 2).all()
        else:
            assert fid.max_err[2, 0 if where == 1 else 2] >= big / 2 and fid.max_ref[2] < 10


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_five_runs_on_two_streams_give_equal_bits(dtype):
    from vorta_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.vorta.*)
    xs = _random_case(3, 1025, DTYPES[dtype], seed=17)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())]
    runs = []
    for i in range(5):
        with torch.cuda.stream(streams[i % 2]):
            runs.append(ops.expert_fidelity(xs[:3], xs[3]))
    torch.cuda.synchronize()
    runs.append(ops.expert_fidelity(xs[:3], xs[3]))  # and the default stream
    torch.cuda.synchronize()
    for r in runs[1:]:
        for name in ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err"):
            assert torch.equal(getattr(r, name), getattr(runs[0], name)), name
    out = torch.ops.vorta.expert_fidelity(xs[0], xs[1], xs[2], xs[3])  # the registered operator: the same launcher
    for got, name in zip(out, ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref")):
        assert torch.equal(got, getattr(runs[0], name)), name


# ------------------------------------------------------------------------------------------------------ operator level
def _golden_case(golden, model, dtype):
    """the G8 / G11 inputs (head dim 16) zero-padded to 128, the scale passed explicitly: scores and outputs unchanged"""
    g8, g = golden("g8_eval_calls"), golden("g11_soft_mixture")

    def pad(x):
        out = torch.zeros(x.shape[:-1] + (128,), dtype=dtype, device=dev())
        out[..., :16] = torch.tensor(x).to(dtype).to(dev())
        return out

    pre = "hy" if model == "hunyuan" else "wan"
    q, k, v = (pad(g8[f"{pre}_{n}"]) for n in "qkv")
    t, te = (int(x) for x in g8["text"]) if model == "hunyuan" else (0, 0)
    geo = tuple(tuple(int(x) for x in g8[n]) for n in ("latent", "tile", "window", "group"))
    return q, k, v, torch.tensor(g["routing_score"]).to(dev()), geo, float(g8["rate"]), t, te


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_soft_mixture_attention_files_the_kernels_statistics(golden, model, dtype):
    """`soft_mixture_attention(..., fidelity=[...])` on the G11 inputs: one ExpertFidelity, bit-equal to the kernel run on the
    `expert_outs` buffers of the same launches and their mix; `out` bit-equal to a call without the keyword; the autograd
    form files the same bits"""
    from vorta_amd import ops
    from vorta_amd.routed import (HeadRouting, geometry_for, routed_attention, soft_mixture_attention,
                                  soft_mixture_attention_autograd)
    q, k, v, sc, (latent, tile, window, group), rate, t, te = _golden_case(golden, model, DTYPES[dtype])
    geom = geometry_for(latent, tile, window, group, rate, dev())
    kw = dict(model=model, text_len=t, text_valid=te, scale=0.25)
    plain = soft_mixture_attention(q, k, v, sc, geom, **kw)
    filed = []
    out = soft_mixture_attention(q, k, v, sc, geom, fidelity=filed, **kw)
    assert torch.equal(out, plain)
    assert len(filed) == 1 and isinstance(filed[0], ops.ExpertFidelity)
    H, N = q.shape[1], q.shape[2]
    bufs = [torch.empty_like(q) for _ in range(3)]
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, dev()), geom, expert_outs=bufs, fp8=False, **kw)
    mixed = ops.mix_experts([b[0] for b in bufs], sc, torch.empty_like(q)[0])
    assert torch.equal(mixed, plain[0])
    direct = ops.expert_fidelity(bufs, mixed)
    for name in ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err"):
        assert torch.equal(getattr(filed[0], name), getattr(direct, name)), name
    assert filed[0].n == direct.n == N * 128
    check(direct, reference([b[0] for b in bufs], mixed), N, f"{dtype} {model} G11 operator")
    rel = direct.rel_error()
    assert rel.shape == (H, 3) and bool(torch.isfinite(rel).all()) and bool((rel[:, :2] > 0).all())
    # the differentiable form: the same forward, the same statistics, and a backward that does not mind the extra argument
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    filed2 = []
    out2 = soft_mixture_attention_autograd(*leaves, geom, model=model, text_len=t, text_valid=te, scale=0.25, fidelity=filed2)
    assert torch.equal(out2.detach(), plain) and len(filed2) == 1
    for name in ("sq_ref", "max_ref", "sq_err", "max_err"):
        assert torch.equal(getattr(filed2[0], name), getattr(direct, name)), name
    out2.float().sum().backward()
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in leaves)


def test_accuracy_summary_written():
    """the largest error over bound of this module's cases (runs after them)"""
    if not RATIOS:
        return
    lines = ["tests/test_hip_expert_fidelity.py: sums of vorta_expert_fidelity against float64 numpy on one MI355X",
             "bound: VORTA_FIDELITY_CHAIN(n_rows) 2^-24, relative (n_rows 1 .. 1025: chain 22 .. 23, bound 1.3e-6 .. 1.4e-6)",
             "largest |sum - exact| / (bound x exact) per case:"]
    lines += [f"  {case}: {r:.4f}" for case, r in RATIOS.items()]
    lines.append(f"largest over all cases: {max(RATIOS.values()):.4f} (maxima: exact in every case)")
    print("\n".join(lines))
    path = os.environ.get("VORTA_EXPERT_FIDELITY_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
