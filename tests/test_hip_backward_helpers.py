"""GPU: the two backward kernels that are not attention, held to exact answers (elsewhere they run only inside end-to-end
autograd tests, where their error drowns in the attention's).

  * vorta_cast_grads: the destination is src.to(dtype) bit for bit -- round to nearest even at exact ties of both parities,
    signed zeros, overflow to +-inf, fp16 and bf16 subnormals, +-inf, NaN where and only where the source has one -- for one,
    two and three tensor pairs in one launch, every pair in a layout of its own, with a partial last workgroup; the pad of a
    destination keeps its sentinel.
  * vorta_mix_experts_bwd: on integer-valued inputs in [-2, 2] every product and partial sum is exact in float32 (|sum| <
    2^24), so dscores must EQUAL the float64 inner products, whatever the split into VORTA_MIX_BWD_PARTS parts and 16-row
    steps; on random inputs two runs give the same bits; no rows give zeros."""
import ctypes

import pytest
import torch

from _util import dev

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
SENTINEL = 7.0


def _specials():
    """float32 values at which a float32 -> 16-bit conversion can go wrong"""
    x = []
    for frac in (2.0 ** -11, 2.0 ** -8):  # half an ulp of fp16 / of bf16 at 1
        for m in range(4):  # the tie above 1 + m ulp: to the even neighbour, down for even m, up for odd m
            x += [1 + (2 * m + 1) * frac, -(1 + (2 * m + 1) * frac), 1 + (2 * m + 1) * frac + 2.0 ** -20,
                  1 + (2 * m + 1) * frac - 2.0 ** -20]
    x += [0.0, -0.0, 1.0, -1.0]
    x += [65504.0, 65519.0, 65520.0, -65520.0, 65536.0, 1e5, -7e4]  # fp16: the largest, under / at the tie to inf, past it
    x += [3.3895313892515355e38, 3.3961775292304601e38, -3.3961775292304601e38, 3.4e38, 3.4028234663852886e38]  # the same, bf16
    x += [2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -25,
          3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26, 1e-7, 6e-8, 5e-6, -3e-6]  # fp16 subnormals, ties among them, to zero
    x += [2.0 ** -126, 2.0 ** -127, 2.0 ** -133, -2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 1.5 * 2.0 ** -134, 2.0 ** -135,
          1e-39, -4e-40, 2.0 ** -149]  # bf16 subnormals (float32 subnormals), ties among them, to zero
    x += [float("inf"), float("-inf"), float("nan"), -float("nan")]
    return torch.tensor(x, dtype=torch.float32)


def _cast_pair(t, heads, n, dtype, gen):
    """(source view, destination view, destination storage, storage -> view) of pair t, each pair with strides of its own"""
    vals = torch.randn((heads, n, 128), generator=gen)
    sp = _specials()
    flat = vals.view(-1)
    flat[:sp.numel()] = sp[torch.randperm(sp.numel(), generator=gen)]
    if flat.numel() >= 3 * sp.numel():
        flat[-sp.numel():] = sp  # in the last, partial workgroup too
    if t == 0:
        src = torch.empty((n, heads, 128), dtype=torch.float32, device=dev()).permute(1, 0, 2)
        dview = lambda b: b[:, 1:n + 1, :128]  # noqa: E731
        base = torch.full((heads, n + 2, 136), SENTINEL, dtype=dtype, device=dev())
    elif t == 1:
        src = torch.empty((heads, n, 132), dtype=torch.float32, device=dev())[..., :128]
        dview = lambda b: b.permute(1, 0, 2)[:, :, 8:136]  # noqa: E731
        base = torch.full((n, heads, 144), SENTINEL, dtype=dtype, device=dev())
    else:
        src = torch.empty((heads + 1, n + 3, 128), dtype=torch.float32, device=dev())[1:, 3:]
        dview = lambda b: b[1:, :, 16:144]  # noqa: E731
        base = torch.full((heads + 1, n, 152), SENTINEL, dtype=dtype, device=dev())
    src.copy_(vals)
    assert torch.equal(src.cpu().view(torch.int32), vals.view(torch.int32))  # (the copy kept every bit, NaN and -0 included)
    return vals, src, dview(base), base, dview


@pytest.mark.parametrize("heads", [1, 5])
@pytest.mark.parametrize("n_rows", [1, 15, 17, 333])
def test_cast_grads_is_torchs_conversion_bit_for_bit(n_rows, heads):
    from vorta_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(100 * n_rows + heads)
    for dtype in DTYPES:
        for n_tensors in (1, 2, 3):
            pairs = [_cast_pair(t, heads, n_rows, dtype, gen) for t in range(n_tensors)]
            ops.cast_grads([p[1] for p in pairs], [p[2] for p in pairs])
            for t, (vals, src, dst, base, dview) in enumerate(pairs):
                what = f"{dtype} rows {n_rows} heads {heads} pair {t} of {n_tensors}"
                want, got = vals.to(dtype), dst.cpu()
                nan = torch.isnan(want)
                assert nan.any() and torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
                a, b = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
                bad = (a != b).nonzero().flatten()[:4]
                assert torch.equal(a, b), (f"{what}: {int((a != b).sum())} elements differ, first from float32 "
                                           f"{vals[~nan][bad].tolist()}: {got[~nan][bad].tolist()} for {want[~nan][bad].tolist()}")
                outside = base.clone()
                dview(outside).fill_(SENTINEL)
                assert (outside == SENTINEL).all(), f"{what}: the destination's pad lost its sentinel"


def test_specials_are_what_they_claim():
    """(the list above, against torch's conversion on the CPU: ties to both parities, overflow, subnormals, signed zero)"""
    sp = _specials()
    for dtype, ulp in ((torch.float16, 2.0 ** -10), (torch.bfloat16, 2.0 ** -7)):
        y = sp.to(dtype)
        tie = torch.tensor([1 + ulp / 2, 1 + 3 * ulp / 2], dtype=torch.float32)
        assert all((sp == t).any() for t in tie)
        assert tie.to(dtype).tolist() == [1.0, 1 + 2 * ulp]  # down to the even neighbour, up to the even neighbour
        finite = torch.isfinite(sp)
        assert (torch.isinf(y) & finite).sum() >= 4  # finite values that overflow
        tiny = torch.finfo(dtype).smallest_normal
        assert ((y != 0) & (y.abs().float() < tiny)).sum() >= 4  # results that are subnormal
        assert ((y == 0) & (sp != 0)).sum() >= 2  # values that round to zero
    z = torch.tensor([-0.0]).to(torch.float16)
    assert z.view(torch.int16).item() == -32768


# ------------------------------------------------------------------------------------------------------ mix_experts_bwd
def _mix_views(vals):
    """the three experts' outputs and d_out (vals: four (H,N,128) tensors on the device), each in a layout of its own"""
    heads, n, _ = vals[0].shape
    dtype = vals[0].dtype
    x0 = torch.empty((n, heads, 128), dtype=dtype, device=dev()).permute(1, 0, 2)
    x1 = torch.full((heads, n + 2, 128), 9.0, dtype=dtype, device=dev())[:, 1:n + 1]
    x2 = torch.full((heads, n, 136), 9.0, dtype=dtype, device=dev())[..., :128]
    g = torch.full((n, 2, heads, 128), 9.0, dtype=dtype, device=dev())[:, 1].permute(1, 0, 2)
    views = (x0, x1, x2, g)
    for a, b in zip(views, vals):
        a.copy_(b)
    return views


@pytest.mark.parametrize("heads", [1, 5])
@pytest.mark.parametrize("n_rows", [1, 7, 33, 384, 1000])
def test_mix_experts_bwd_is_exact_on_integers(n_rows, heads):
    from vorta_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(10 * n_rows + heads)
    for dtype in DTYPES:
        vals = [torch.randint(-2, 3, (heads, n_rows, 128), generator=gen).to(dtype).to(dev()) for _ in range(4)]
        x0, x1, x2, g = _mix_views(vals)
        got = ops.mix_experts_bwd([x0, x1, x2], g)
        want = torch.stack([(vals[3].double() * vals[e].double()).sum((1, 2)) for e in range(3)], dim=1)
        assert want.abs().max() < 2 ** 24 and want.any()
        assert got.dtype == torch.float32 and tuple(got.shape) == (heads, 3)
        assert torch.equal(got.double(), want), f"{dtype} rows {n_rows} heads {heads}: {got.tolist()} for {want.tolist()}"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_mix_experts_bwd_same_bits_on_every_run(dtype):
    from vorta_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(5)
    vals = [torch.randn((5, 1000, 128), generator=gen).to(dtype).to(dev()) for _ in range(4)]
    x0, x1, x2, g = _mix_views(vals)
    first = ops.mix_experts_bwd([x0, x1, x2], g)
    want = torch.stack([(vals[3].double() * vals[e].double()).sum((1, 2)) for e in range(3)], dim=1)
    # 128000 products of unit variance, summed in float32: the rounding error is far under 1e-3 of the sum's spread, sqrt(128000)
    assert (first.double() - want).abs().max() <= 1e-3 * 128000 ** 0.5
    for _ in range(3):
        assert torch.equal(ops.mix_experts_bwd([x0, x1, x2], g), first)


def test_mix_experts_bwd_of_no_rows_is_zero():
    """n_rows = 0 through the C entry point (a torch view without rows has no address to pass): dscores is written, all zero"""
    from vorta_amd import _C, ops
    heads = 5
    xs = [torch.ones((heads, 4, 128), dtype=torch.bfloat16, device=dev()) for _ in range(4)]
    dscores = torch.full((heads, 3), SENTINEL, dtype=torch.float32, device=dev())
    ws = torch.full((heads * _C.MIX_BWD_PARTS * 4,), SENTINEL, dtype=torch.float32, device=dev())
    a = _C.MixBwdArgs()
    a.struct_size = ctypes.sizeof(_C.MixBwdArgs)
    a.dtype, a.head_dim, a.heads, a.n_experts, a.n_rows = _C.VORTA_BF16, 128, heads, 3, 0
    for e in range(3):
        a.x[e] = ops._tensor(xs[e])
    a.d_out = ops._tensor(xs[3])
    a.dscores, a.ws = dscores.data_ptr(), ws.data_ptr()
    _C.check(_C.lib().vorta_mix_experts_bwd(ctypes.byref(a), ops._stream()), "vorta_mix_experts_bwd")
    torch.cuda.synchronize()
    assert not dscores.any()
