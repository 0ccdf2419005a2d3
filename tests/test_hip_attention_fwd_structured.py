"""GPU: the 16-bit attention forward (csrc/attn_fwd.hip: the pipelined kernel, the plain kernel of variant 1, the fused grid
and the split-key merge) on structured inputs, held to its own rounding model (tests/_attn_fwd_model.py) row by row and
channel by channel instead of to a tolerance over the whole tensor.

Inputs: white noise, peaked local heads, redundant heads with tied scores, score rows +-100 from zero, keys that lift the
running maximum late, a staircase of key norms that raises the loop's reference point block after block, values with a
common part; bf16 and fp16.  Launches: dense at both workgroup sizes, with tails and row offsets, with 3 and 8 key splits (two
of the 8 empty), through strided (S, H, D) storage, the two gather launches of the backward tests with and without splits,
variant 1, key counts that reach every step-parity and tail path of the loop, and three launches as one fused grid.

Rule, errors as absolute 2-norms against the float64 output (no division: rows of tiny norm need no special case):

    whole tensor                                   e_hip <= 2 e_model + 4 e_f32      (the rule of the backward tests)
    every written query row (128 channels)         e_hip <= 3 e_model + 4 e_f32      (lane & 31 is the query: a wrong lane)
    every channel (the written rows of a head)     e_hip <= 3 e_model + 4 e_f32      (a wrong accumulator register or v_rd column)

e_model: float64 everywhere but the three roundings the kernel makes by design (Q scale log2 e, P, out).  e_f32: a plain
float32 forward; tests/test_host_forward_model.py holds it under e_model / 4 on every case, and holds a float32 emulation of
the loop under 0.9 of all three bounds -- that is where the factor 3 comes from, never from what the kernel gives.  Kernel and
model round P relative to different reference points, so they agree statistically and the rule compares errors, not outputs.

Exact, as bits: rows the launch does not name keep the sentinel, positions >= the effective q_valid are zero, every duplicate
row equals its source row, and a fused grid writes what its launches write alone.

Measured on an MI355X: profiles/attn_fwd_structured_accuracy.txt."""
import os

import numpy as np
import pytest
import torch

import _attn_fwd_model as F
import _random_launch as RL
from _util import dev

pytestmark = pytest.mark.gpu

RATIOS = {}  # (family, dtype name, launch, unit) -> e_hip / bound of every unit of the case
IDS = dict(ids=F.dtype_name)


def _bits(x):
    return x.contiguous().view(torch.int16)


def _fresh(shape, dtype):
    return torch.full(shape, RL.SENTINEL, dtype=dtype, device=dev())


def _check(got, c, what, key, rows=None):
    """the three rules and the exact checks of one output (a CPU tensor) against the references of case c; `rows`: (H,S)
    mask of the rows the rules look at (default: every row at a position below q_valid)"""
    assert torch.isfinite(got.float()).all(), f"{what}: the output is not finite"
    valid, zero, dups = c["valid"], c["zero"], c["dups"]
    sentinel = torch.tensor(RL.SENTINEL, dtype=got.dtype)
    untouched = ~(valid | zero | dups)
    assert (_bits(got[untouched]) == _bits(sentinel.reshape(1))).all(), f"{what}: wrote rows the launch does not name"
    assert not _bits(got[zero]).any(), f"{what}: positions past q_valid are not zero bits"
    for h, dst, src in F.dup_pairs(c["kw"], c["H"]):
        assert torch.equal(_bits(got[h, dst]), _bits(got[h, src])), f"{what}: a duplicate row differs from its source"
    if rows is not None:
        c = dict(c, valid=rows)
    r = F.unit_ratios(got, c)
    for unit, x in r.items():
        x = x.reshape(-1)
        RATIOS.setdefault(key + (unit,), []).extend(x.tolist())
        print(f"{what} {unit}: e_hip / bound max {float(x.max()):.3f} median {float(x.median()):.3f} over {x.numel()}")
    for unit, x in r.items():
        worst = int(x.reshape(-1).argmax())
        assert float(x.max()) <= 1.0, f"{what}: {unit} {worst} is at {float(x.max()):.3f} of its bound"


def _operands(c, which, dtype):
    """q, k, v and a sentinel-filled out on the device; (S, H, D) storage views for the strided launch"""
    H, S = c["H"], c["S"]
    if which != "dense_strided":
        return tuple(c[n].to(dev()) for n in ("q", "k", "v")) + (_fresh((H, S, 128), dtype),)
    qkv = torch.stack([c[n].permute(1, 0, 2) for n in ("q", "k", "v")]).contiguous().to(dev())  # (3, S, H, D)
    q, k, v = (qkv[i].permute(1, 0, 2) for i in range(3))
    out = _fresh((S, H, 128), dtype).permute(1, 0, 2)
    assert q.stride(1) == H * 128 and out.stride(1) == H * 128
    return q, k, v, out


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
@pytest.mark.parametrize("fam,which", [fw for fw in F.CASES if fw[1] not in F.FUSED])
def test_structured_inputs(fam, which, dtype):
    from vorta_amd import ops
    c = F.case(fam, dtype, which)  # the references: computed once on the CPU, never from the library
    kw = F.launch(which, dev())[2]
    q, k, v, out = _operands(c, which, dtype)
    ops.attn_fwd(q, k, v, out, **kw)
    torch.cuda.synchronize()
    _check(out.cpu(), c, f"{fam} {F.dtype_name(dtype)} {which}", (fam, F.dtype_name(dtype), which))


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
@pytest.mark.parametrize("fam", F.FAMILIES)
def test_fused_grid(fam, dtype, monkeypatch):
    """a dense launch, one with a key table of 7 blocks and 12 keys and one with three key splits, 256-row workgroups over
    one operand set, as ONE grid through ops.attn_fwd_batch: each output meets the rule and is bit-equal to its launch alone"""
    from vorta_amd import ops
    cases = [F.case(fam, dtype, which) for which in F.FUSED]
    q, k, v = (cases[0][n].to(dev()) for n in ("q", "k", "v"))
    kws = [F.launch(which, dev())[2] for which in F.FUSED]
    fused, alone = ([_fresh(q.shape, dtype) for _ in F.FUSED] for _ in range(2))
    single = []
    real_one = ops._launch_one
    monkeypatch.setattr(ops, "_launch_one", lambda a: (single.append(a), real_one(a)))
    ops.attn_fwd_batch([dict(q=q, k=k, v=v, out=o, **kw) for o, kw in zip(fused, kws)])
    torch.cuda.synchronize()
    assert not single, "every segment resolves to the 256-row pipelined kernel: the batch is one fused grid"
    for o, kw in zip(alone, kws):
        ops.attn_fwd(q, k, v, o, **kw)
    torch.cuda.synchronize()
    for which, c, o, a in zip(F.FUSED, cases, fused, alone):
        assert torch.equal(_bits(o), _bits(a)), f"{fam} {which}: the fused grid and the launch alone write different bits"
        _check(o.cpu(), c, f"{fam} {F.dtype_name(dtype)} {which}", (fam, F.dtype_name(dtype), which))


@pytest.mark.parametrize("form", ("pipelined", "three splits", "variant 1"))
@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
def test_rows_past_q_valid_are_zeros_whatever_q_holds(dtype, form):
    """include/vorta_hip.h: positions at or past q_valid "are written as zeros".  q_valid = 300 cuts the wave of positions
    288 .. 319; its rows past the cut hold inf and NaN in q, whose accumulators are NaN.  The output there is zero bits
    (0 x NaN would be NaN: the epilogues and the split-key merge select on the position), and the twelve rows of that wave
    before the cut, which share its rescale decisions, still meet the rule like every other row"""
    from vorta_amd import ops
    which = "dense_qvalid_v1" if form == "variant 1" else "dense_qvalid"
    c = F.case("white", dtype, which)
    kw = dict(F.launch(which, dev())[2], n_splits=3 if form == "three splits" else 1)
    q = c["q"].clone()
    q[0, 300:320:2] = float("inf")
    q[0, 301:320:4] = float("nan")
    q[0, 303:320:4] = -float("inf")
    q[0, 310, 5:] = 1.0  # (and a row with one NaN among finite numbers)
    q[0, 310, 0] = float("nan")
    out = _fresh(q.shape, dtype)
    ops.attn_fwd(q.to(dev()), c["k"].to(dev()), c["v"].to(dev()), out, **kw)
    torch.cuda.synchronize()
    got = out.cpu()
    assert not _bits(got[0, 300:]).any(), "rows past q_valid are not zero bits"
    _check(got, c, f"white {F.dtype_name(dtype)} q_valid in a wave, {form}", ("white", F.dtype_name(dtype), f"nan_rows {form}"))
    wave = torch.zeros_like(c["valid"])
    wave[0, 288:300] = True
    _check(got, c, f"white {F.dtype_name(dtype)} the wave of the cut, {form}", ("white", F.dtype_name(dtype), f"nan_wave {form}"), rows=wave)


@pytest.mark.parametrize("form", ("pipelined", "three splits", "variant 1"))
@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
def test_nan_below_q_valid_stays_nan(dtype, form):
    """the zeros are a matter of the POSITION alone.  A NaN in the q row of a position below q_valid gives a NaN output row
    (its row sum is NaN) and leaves the other rows of its wave to the rule; a NaN in one key row gives every position below
    q_valid a NaN row.  Neither is turned into zeros, and the positions past q_valid are zero bits in both"""
    from vorta_amd import ops
    which = "dense_qvalid_v1" if form == "variant 1" else "dense_qvalid"
    c = F.case("white", dtype, which)
    kw = dict(F.launch(which, dev())[2], n_splits=3 if form == "three splits" else 1)
    what = f"white {F.dtype_name(dtype)} NaN below q_valid, {form}"
    q = c["q"].clone()
    q[0, 100, 7] = float("nan")
    out = _fresh(q.shape, dtype)
    ops.attn_fwd(q.to(dev()), c["k"].to(dev()), c["v"].to(dev()), out, **kw)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[0, 100].float()).all(), f"{what}: the row of the NaN query is not NaN"
    assert not _bits(got[0, 300:]).any()
    got[0, 100] = c["model"][0, 100].to(dtype)  # (taken out of the rule: every other row meets it)
    _check(got, c, what, ("white", F.dtype_name(dtype), f"nan_q_valid_row {form}"))
    k = c["k"].clone()
    k[0, 200, 3] = float("nan")
    out = _fresh(q.shape, dtype)
    ops.attn_fwd(c["q"].to(dev()), k.to(dev()), c["v"].to(dev()), out, **kw)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[0, :300].float()).all(), f"{what}: a NaN key row did not reach every output row"
    assert not _bits(got[0, 300:]).any(), f"{what}: positions past q_valid are not zero bits"


def test_accuracy_summary_written():
    """max / median of e_hip / bound per (family, dtype, launch, unit) over this module's cases (runs after them;
    profiles/attn_fwd_structured_accuracy.txt comes from here when VORTA_FWD_STRUCTURED_ACCURACY_OUT names a file)"""
    if not RATIOS:
        return  # (selected on its own: nothing to summarise)
    lines = []
    for (fam, dn, which, unit), r in sorted(RATIOS.items()):
        r = np.array(r)
        lines.append(f"{fam} {dn} {which} {unit}: units {len(r)} e_hip / bound max {r.max():.3f} median {float(np.median(r)):.3f}")
    for unit in ("tensor", "row", "channel"):  # the figures of DESIGN.md 5
        for dn in map(F.dtype_name, F.DTYPES):
            r = np.array([x for (f, d, w, u), rs in RATIOS.items() if u == unit and d == dn for x in rs])
            if len(r):
                lines.append(f"all families and launches {dn} {unit}: units {len(r)} e_hip / bound max {r.max():.3f} "
                             f"median {float(np.median(r)):.3f}")
    print("\n".join(lines[-6:]))
    path = os.environ.get("VORTA_FWD_STRUCTURED_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / bound of the 16-bit attention forward over the cases of tests/test_hip_attention_fwd_structured.py "
                    "(bounds: tensor 2 e_model + 4 e_f32, row and channel 3 e_model + 4 e_f32; absolute 2-norms against "
                    "float64)\n" + "\n".join(lines) + "\n")
