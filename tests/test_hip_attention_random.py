"""Random launches of the three 8-bit attention families against the launch emulator, and random fused grids of all four
families against their stand-alone launches and their references (tests/_random_launch.py draws the geometry).

  fp8  all e4m3 (csrc/attn_fwd_fp8.hip): q, k, v from ops.fp8_quantize_qkv;
  mx   16-bit scores, e4m3 P V (csrc/attn_fwd_mx.hip): 16-bit q, k, v from ops.fp8_quantize_v;
  i8   int8 scores, e4m3 P V (csrc/attn_fwd_i8.hip): 16-bit q, k from ops.i8_quantize_k, e4m3 v;
  16   16 bits (csrc/attn_fwd.hip), in the fused-grid tests only (its single launches: tests/test_hip_attention.py).

The 8-bit kernels are held to O.fp8_attn_launch on the same operands with the tolerance of the family tests
(tests/test_hip_fp8.py `_check`, with the emulator's rounding-midpoint slack); split boundaries are cut from the host n_kv
(`split_n_kv`) while the keys stop at the device length, as the kernels do."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O

pytestmark = pytest.mark.gpu

import _random_launch as R  # noqa: E402
from _util import ATOL_SAME, dev, rounded, to_dev  # noqa: E402
from test_hip_fp8 import _check, _decoded, _vmax  # noqa: E402
from test_hip_i8 import _hooks, _vdec  # noqa: E402
from test_hip_mx import MX, _operands as _mx_operands  # noqa: E402

FAMILIES = ("16", "fp8", "mx", "i8")


class Family:
    """one operand set of a family over (H, S, 128) buffers: its launch keywords and its reference"""

    def __init__(self, name, rng, H, S, dtype):
        from vorta_amd import ops
        self.name, self.dtype = name, dtype
        x = [rng.standard_normal((H, S, 128)) for _ in range(3)]
        if name == "i8":
            x[0] = x[0] + 0.7 * rng.standard_normal((1, 1, 128))  # a query centre for the int8 conversion to take out
        qd, kd, vdev = (to_dev(a, dtype) for a in x)
        if name == "16":
            self.ops_kw = dict(q=qd, k=kd, v=vdev)
            self.r = [rounded(a, dtype) for a in x]
        elif name == "fp8":
            f8 = ops.fp8_quantize_qkv(qd, kd, vdev)
            self.ops_kw = dict(q=f8.q, k=f8.k, v=f8.v, v_descale=f8.v_descale)
            self.q8, self.k8, self.v8, self.vd = _decoded(f8)
        elif name == "mx":
            v8, vd, _ = ops.fp8_quantize_v(vdev)
            self.ops_kw = dict(q=qd, k=kd, v=v8, v_descale=vd)
            self.q8, self.k8, self.v8, self.vd = _mx_operands(qd, kd, v8, vd, dtype)
        else:
            i8 = ops.i8_quantize_k(qd, kd)
            v8, vd, _ = ops.fp8_quantize_v(vdev)
            self.ops_kw = dict(q=qd, k=i8.k8, v=v8, v_descale=vd, i8=i8)
            self.hooks = _hooks(qd, i8)
            self.v8, self.vd = _vdec(v8, vd)
        self.out_shape = (H, S, 128)

    def call(self, out, L, **over):
        """ops.attn_fwd / attn_fwd_batch keywords of launch L writing `out`"""
        return dict(self.ops_kw, out=out, **R.kwargs(L, dev(), **over))

    def fresh_out(self):
        return torch.full(self.out_shape, R.SENTINEL, dtype=self.dtype, device=dev())

    def check(self, out, L, what=""):
        """out against the float64 oracle (16 bits) or the launch emulator (8 bits); every row L does not name holds the
        sentinel"""
        desc = dict(R.describe(L), family=self.name, what=what)
        if self.name == "16":
            ref = R.dense_reference(L, *self.r, lambda q, k, v: O.dense_attention(q[None], k[None], v[None])[0])
            err = float(np.abs(out.float().cpu().numpy() - ref).max())
            assert err <= ATOL_SAME[self.dtype], (err, desc)
            return
        H, S, _ = self.out_shape
        ref, amb = np.full(self.out_shape, R.SENTINEL), np.zeros((H, S))
        kw = R.emulator_kwargs(L)
        for h in L.live:
            if self.name == "i8":
                O.fp8_attn_launch(None, None, self.v8[h], ref[h], self.vd[h], ambiguous=amb[h], wave_operands=self.hooks[h],
                                  p_mode="mx", defer=24.0, **kw)
            else:
                O.fp8_attn_launch(self.q8[h], self.k8[h], self.v8[h], ref[h], self.vd[h], ambiguous=amb[h],
                                  **(MX if self.name == "mx" else {}), **kw)
        try:
            _check(out, ref, self.dtype, amb, _vmax(self.v8, self.vd))
        except AssertionError as e:
            raise AssertionError(f"{e} {desc}") from None


def _launch(fam, out, L, **over):
    from vorta_amd import ops
    kw = fam.call(out, L, **over)
    ops.attn_fwd(kw.pop("q"), kw.pop("k"), kw.pop("v"), kw.pop("out"), **kw)


@pytest.mark.parametrize("family", ["fp8", "mx", "i8"])
@pytest.mark.parametrize("seed", range(16))
def test_8bit_random_launches_vs_emulator(family, seed):
    """Random geometry -- key splits 1..8 with query groups, q_block_table, row tables, duplicates, q_valid tails, head lists,
    n_heads_dev (0 included), device n_kv / q_valid (empty last splits included), both workgroup sizes -- against the
    emulator.  With one split, device lengths L, V write the bytes of host lengths L, V."""
    rng = np.random.default_rng(7000 + 100 * FAMILIES.index(family) + seed)
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    L = R.draw(rng, S_range=(64, 600), empty_tail=seed % 4 == 3)
    fam = Family(family, rng, L.H_buf, L.S, dtype)
    out = fam.fresh_out()
    _launch(fam, out, L)
    torch.cuda.synchronize()
    fam.check(out, L)
    if L.n_splits == 1 and (L.n_kv_dev is not None or L.q_valid_dev is not None):
        host = fam.fresh_out()
        _launch(fam, host, L, n_kv=L.n_kv_eff, q_valid=L.q_valid_eff, n_kv_dev=None, q_valid_dev=None)
        assert torch.equal(host, out), R.describe(L)


def _segments(rng, n, H, S):
    """n random 256-row launches over one (H, S) operand set; each writes its own output tensor"""
    segs = []
    for _ in range(n):
        L = R.draw(rng, H_buf=H, S=S, block_rows=256)
        if rng.integers(0, 4) == 0:
            L.n_heads_dev, L.live = 0, L.heads[:0]  # a segment whose every slot is dead
        segs.append(L)
    return segs


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed", range(5))
def test_random_fused_grids_match_separate_launches_and_reference(family, seed, monkeypatch):
    """2..6 random segments (splits or none, duplicates, head lists, n_heads_dev down to no live slot, device lengths) as ONE
    fused grid through ops.attn_fwd_batch: the bytes of each segment launched alone with 256-row workgroups and the same
    splits, and the reference of each segment"""
    from vorta_amd import ops
    rng = np.random.default_rng(9000 + 100 * FAMILIES.index(family) + seed)
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    H, S = int(rng.integers(1, 5)), int(rng.integers(200, 600))
    fam = Family(family, rng, H, S, dtype)
    segs = _segments(rng, int(rng.integers(2, 7)), H, S)
    fused = [fam.fresh_out() for _ in segs]
    single = []
    real_one = ops._launch_one
    monkeypatch.setattr(ops, "_launch_one", lambda a: (single.append(a), real_one(a)))
    ops.attn_fwd_batch([fam.call(o, L) for o, L in zip(fused, segs)])
    torch.cuda.synchronize()
    assert not single, "every segment resolves to the 256-row pipelined kernel: the batch is one fused grid"
    alone = [fam.fresh_out() for _ in segs]
    for o, L in zip(alone, segs):
        _launch(fam, o, L)
    torch.cuda.synchronize()
    for i, (o, a, L) in enumerate(zip(fused, alone, segs)):
        assert torch.equal(o, a), (i, R.describe(L))
        fam.check(o, L, what=f"segment {i} of {len(segs)}")


@pytest.mark.parametrize("family", FAMILIES)
def test_seven_launches_are_not_fused(family, monkeypatch):
    """VORTA_MAX_FUSED_LAUNCHES is 6: the C entry refuses 7 segments (VORTA_EINVAL) and ops.attn_fwd_batch launches 7 fusable
    calls one by one -- the bytes of the stand-alone launches"""
    from vorta_amd import _C, ops
    rng = np.random.default_rng(9500 + FAMILIES.index(family))
    dtype = torch.bfloat16
    H, S = 3, 400
    fam = Family(family, rng, H, S, dtype)
    segs = _segments(rng, 7, H, S)
    outs = [fam.fresh_out() for _ in segs]
    built = []
    for o, L in zip(outs, segs):
        kw = fam.call(o, L)
        built.append(ops._attn_args(kw.pop("q"), kw.pop("k"), kw.pop("v"), kw.pop("out"), **kw))
    args = [a for a, _ in built]
    arr = (_C.AttnArgs * 7)(*args)
    ext = () if args[0]._ext is None else (C.byref(args[0]._ext),)
    assert getattr(_C.lib(), args[0]._family.batch)(arr, *ext, 7, ops._stream()) == _C.VORTA_EINVAL
    assert all(torch.all(o == R.SENTINEL) for o in outs)  # refused before anything ran
    single = []
    real_one = ops._launch_one
    monkeypatch.setattr(ops, "_launch_one", lambda a: (single.append(a), real_one(a)))
    ops.attn_fwd_batch([fam.call(o, L) for o, L in zip(outs, segs)])
    torch.cuda.synchronize()
    assert len(single) == 7
    monkeypatch.setattr(ops, "_launch_one", real_one)
    for i, (o, L) in enumerate(zip(outs, segs)):
        a = fam.fresh_out()
        _launch(fam, a, L)
        torch.cuda.synchronize()
        assert torch.equal(o, a), (i, R.describe(L))
    fam.check(outs[0], segs[0])


def test_fused_grid_refuses_segments_with_other_8bit_operands():
    """a fused grid takes ONE operand set (the first launch's ext): segments with another v_descale, other options or other
    int8 key operands are refused on the host instead of being computed with the first segment's"""
    from vorta_amd import ops
    rng = np.random.default_rng(9900)
    H, S = 2, 300
    L = R.draw(rng, H_buf=H, S=S, block_rows=256, device_lengths=False)
    for name in ("fp8", "mx", "i8"):
        fam = Family(name, rng, H, S, torch.bfloat16)
        out = [fam.fresh_out() for _ in range(2)]
        other_vd = fam.ops_kw["v_descale"].clone()
        bad = [dict(v_descale=other_vd), dict(fp8_opts=dict(defer=2.0) if name == "fp8" else dict(defer=20.0))]
        if name == "i8":
            i8 = fam.ops_kw["i8"]
            bad += [dict(i8=ops.I8Operands(i8.k8, i8.k_bias.clone(), i8.q_prep, i8.k_head_scale, i8.ws)),
                    dict(i8=ops.I8Operands(i8.k8, i8.k_bias, i8.q_prep.clone(), i8.k_head_scale, i8.ws)),
                    dict(i8=ops.I8Operands(i8.k8, i8.k_bias, i8.q_prep, i8.k_head_scale.clone(), i8.ws))]
        for b in bad:
            with pytest.raises(ValueError, match="operand"):
                ops.attn_fwd_batch([fam.call(out[0], L), dict(fam.call(out[1], L), **b)])
        torch.cuda.synchronize()
        assert all(torch.all(o == R.SENTINEL) for o in out), name  # nothing was launched
        ops.attn_fwd_batch([fam.call(out[0], L), fam.call(out[1], L)])  # the same operand set fuses
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1]), name
