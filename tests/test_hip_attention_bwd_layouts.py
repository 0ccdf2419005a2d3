"""GPU: the five attention-backward entry points with every operand in a layout of its own.  The ABI gives q, k, v, o, d_o,
dq, dk and dv each a stride_h / stride_s (16-bit elements for the first five, floats for the gradients); every other backward
test passes eight contiguous (H,S,128) tensors, where any two of those fields can be swapped unnoticed.

Each launch runs twice: on contiguous tensors, and on views that hold the same values --

    q, k, v   slices of one packed (S, 3, H, 128) projection buffer (stride_s = 3 H 128, stride_h = 128)
    o         (S, H, 128) permuted                d_o   (H, S + 8, 128)[:, 4:S + 4]
    dq        (H, S, 160) float32 [..., :128]     dk    (S, H, 128) float32 permuted
    dv        (H + 1, S + 5, 128) float32 [1:, :S]
    do_scale  column 1 of an (H, 3) matrix        stats  with two more head slots than the launch uses

-- with the whole storage under dq / dk / dv filled with 3.0 first.  The outputs without atomics (the statistics, attn_bwd_dq's
dq, attn_bwd_dkv's dk / dv, vorta_attn_bwd's dq) must carry the bits of the contiguous run; the outputs summed with float
atomics (vorta_attn_bwd's dk / dv, all of key-major) hold the bound of tests/test_hip_attention_bwd.py against float64 and its
"sentinel + gradient" tolerance; and every element of the storage outside the views -- pad columns, the extra head, the
extra rows -- still equals 3.0."""
import numpy as np
import pytest
import torch

import _random_launch as RL
import test_hip_attention_bwd as B
import test_hip_attention_bwd_key_major as KM
from _attn_restate import named_rows
from _util import dev

pytestmark = pytest.mark.gpu

H, S = 3, 480
# seeds of RL.draw(default_rng(seed), H_buf=3, S=480), chosen by their geometry: every one has live heads, queries below
# q_valid and several key blocks; between them all three heads and head lists of one and two, equal groups and block tables,
# row tables and offsets, duplicate rows, both device lengths
SEEDS = (2003, 2004, 2006, 2014, 2017, 2028)
ALGORITHMS = ("query_major", "key_major", "deterministic")
ATOMIC_FREE = {"query_major": ("dq",), "key_major": (), "deterministic": ("dq", "dk", "dv")}


def _grad_views(fill):
    """([dq, dk, dv] views of shape (H,S,128), their storages, storage -> view) with every storage element = fill"""
    view = (lambda b: b[..., :128], lambda b: b.permute(1, 0, 2), lambda b: b[1:, :S])
    bases = [torch.full(shape, fill, dtype=torch.float32, device=dev())
             for shape in ((H, S, 160), (S, H, 128), (H + 1, S + 5, 128))]
    return [f(b) for f, b in zip(view, bases)], bases, view


def _operand_views(q, k, v, out, d_o, w):
    packed = torch.full((S, 3, H, 128), 5.0, dtype=q.dtype, device=dev())
    for i, x in enumerate((q, k, v)):
        packed[:, i] = x.permute(1, 0, 2)
    qv, kv, vv = (packed[:, i].permute(1, 0, 2) for i in range(3))
    ov = torch.empty((S, H, 128), dtype=q.dtype, device=dev()).permute(1, 0, 2)
    ov.copy_(out)
    gbase = torch.full((H, S + 8, 128), 5.0, dtype=q.dtype, device=dev())
    gv = gbase[:, 4:S + 4]
    gv.copy_(d_o)
    wbase = torch.full((H, 3), 5.0, dtype=q.dtype, device=dev())
    wbase[:, 1] = w
    views = (qv, kv, vv, ov, gv, wbase[:, 1])
    for a, b in zip(views, (q, k, v, out, d_o, w)):
        assert torch.equal(a, b) and (a.dim() == 1 or not a.is_contiguous())
    assert qv.stride() == (128, 3 * H * 128, 1) and ov.stride() == (128, H * 128, 1) and gv.stride() == ((S + 8) * 128, 128, 1)
    return views


def _run(algorithm, q, k, v, out, d_o, bufs, w, kw, n_slots):
    """one algorithm into bufs; the statistics it used (zero-initialised, n_slots head slots), or None"""
    from vorta_amd import ops
    if algorithm == "query_major":
        ops.attn_bwd(q, k, v, out, d_o, *bufs, do_scale=w, **kw)
        return None
    stats = torch.zeros((n_slots, kw["n_q"], 2), dtype=torch.float32, device=dev())
    assert ops.attn_bwd_stats(q, k, v, out, d_o, stats, do_scale=w, **kw) is stats
    if algorithm == "key_major":
        ops.attn_bwd_key_major(q, k, v, out, d_o, *bufs, stats, do_scale=w, **kw)
    else:
        ops.attn_bwd_dq(q, k, v, out, d_o, bufs[0], stats, do_scale=w, **kw)
        ops.attn_bwd_dkv(q, k, v, out, d_o, bufs[1], bufs[2], stats, do_scale=w, **kw)
    return stats


@pytest.mark.parametrize("i", range(len(SEEDS)))
def test_every_operand_in_its_own_layout(i):
    from vorta_amd import ops
    dtype = (torch.bfloat16, torch.float16)[i % 2]
    L = RL.draw(np.random.default_rng(SEEDS[i]), H_buf=H, S=S)
    assert len(L.live) > 0 and L.q_valid_eff > 0
    kw = RL.kwargs(L, dev())
    shape = (H, S, 128)
    q, k, v, d_o, w = KM._inputs(shape, dtype, SEEDS[i], True)
    out = torch.zeros(shape, dtype=dtype, device=dev())
    ops.attn_fwd(q, k, v, out, **kw)
    ref, t16 = KM._references(kw, q, k, v, d_o, w, dtype)
    views = _operand_views(q, k, v, out, d_o, w)
    qm, km = named_rows(kw, shape)
    n_slots = len(L.heads)
    for algorithm in ALGORITHMS:
        what = f"seed {SEEDS[i]} {algorithm} {RL.describe(L)}"
        zero = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
        _run(algorithm, q, k, v, out, d_o, zero, w, kw, n_slots)
        plain = [torch.full(shape, 3.0, dtype=torch.float32, device=dev()) for _ in range(3)]
        stats_plain = _run(algorithm, q, k, v, out, d_o, plain, w, kw, n_slots)
        strided, bases, view = _grad_views(3.0)
        stats_strided = _run(algorithm, *views[:5], strided, views[5], kw, n_slots + 2)
        if stats_plain is not None:
            assert stats_plain[:len(L.live)].any()
            assert torch.equal(stats_strided[:n_slots], stats_plain), f"{what}: the statistics depend on the operands' layout"
            assert not stats_strided[n_slots:].any(), f"{what}: the statistics pass wrote head slots the launch does not have"
        for name, z, p, s, base, f, t, r in zip(("dq", "dk", "dv"), zero, plain, strided, bases, view, t16, ref):
            assert r.any()
            untouched = ~(qm if name == "dq" else km).to(dev())
            assert (s[untouched] == 3.0).all(), f"{what}: {name} disturbed the sentinel of unnamed rows"
            if name in ATOMIC_FREE[algorithm]:
                assert torch.equal(s - 3.0, p - 3.0), f"{what}: {name} depends on the operands' layout"
            else:
                assert torch.allclose(s, z + 3.0, rtol=1e-5, atol=1e-5), f"{what}: {name} is not sentinel + gradient"
                B._bound(name, s.double() - 3.0, t, r, what)  # (float32 at magnitude 3: 2.4e-7 absolute, far under the bound)
            outside = base.clone()
            f(outside).fill_(3.0)
            assert (outside == 3.0).all(), f"{what}: {name} wrote storage outside its view"
