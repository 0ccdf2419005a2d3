"""GPU, bit for bit: the three 8-bit attention forwards -- all e4m3 (csrc/attn_fwd_fp8.hip), 16-bit scores with e4m3 P V
(attn_fwd_mx.hip), int8 scores with e4m3 P V (attn_fwd_i8.hip) -- on inputs whose every softmax row is ONE key
(tests/_attn8_onehot_inputs.py).  The output row of a query is then decode(v8[its key]) x v_descale[head] with every bit equal,
so the routing of a launch -- q_rows, kv_rows, groups, q_block_table, dup_rows, head lists, device lengths, key splits and
their merge -- the P V pipeline behind the scores and the per-(head, channel) v_descale of the epilogue are checked exactly,
not within the tolerance of the Gaussian tests: a key list read one entry off, the last key dropped, a row of one lane written
to another, a split merged with the wrong weight, a scale of the neighbouring head or channel all change bits.

Why the kernels are exact here, per family (tests/test_host_attention_onehot_8bit.py decides the same on the launch emulator,
with no row left out, before any of this runs).  The chosen key leads every other by >= 160 log2 units on the operands the
kernel multiplies (asserted before each launch), so every other probability and every rescale factor is exp2(<= -155): 0 in
float32 and as an e4m3 byte.
  fp8  integer scores; the reference point moves to the block maximum itself: the chosen key's probability is 2^p_bias.
  mx   scores in steps of 20 (A8.SCALE makes q' = round16(q scale log2 e) = +-2); the reference point moves by whole binades:
       the probability is a power of two, an exact e4m3 byte under an exact scale code.
  i8   the same steps through the hand-built head scale, to 1e-7: the byte lands on a power of two.
The row sum (on the MFMA pipe against a tile of ones, or on the VALU with flags = 1) is that power of two, 1.f / l_tot is exact,
and the product with v_descale, a power of two, has the 4 significant bits of an e4m3 value: exact in bf16 and fp16.

Random launches: 16 per family, the dtypes alternating, the workgroup size from the draw, `torch.equal` on the whole buffer --
computed rows, zero bits past q_valid, the sentinel everywhere else.  Options that must not change a bit run beside the
default (A8.options).  Ties: 2 and 4 keys share one k row; the row is the mean of their decoded v rows.  Fused grids: 2 .. 6
launches over one set of keys, values and scales (each with the queries of its own one-hot rows) as one grid."""
import pytest
import torch

import _attn8_onehot_inputs as A8
import _attn_onehot_inputs as OH
import _random_launch as RL
from _util import dev

pytestmark = pytest.mark.gpu


def _call(c, out, **over):
    """ops.attn_fwd / attn_fwd_batch keywords of the case's launch writing `out`"""
    from vorta_amd import ops
    d = c.device(dev())
    if c.family == "i8":
        d["i8"] = ops.I8Operands(*d["i8"])
    if c.family != "fp8":
        d["scale"] = A8.SCALE
    return dict(d, out=out, **RL.kwargs(c.L, dev(), **over))


def _launch(c, out, **over):
    from vorta_amd import ops
    kw = _call(c, out, **over)
    ops.attn_fwd(kw.pop("q"), kw.pop("k"), kw.pop("v"), kw.pop("out"), **kw)


def _fresh(c):
    return torch.full((c.L.H_buf, c.L.S, 128), RL.SENTINEL, dtype=c.dtype, device=dev())


def _assert_bits(out, want, what):
    got = out.cpu()
    bad = (got != want).any(-1).nonzero().tolist()
    assert torch.equal(got, want), f"{what}: {len(bad)} rows differ, first (head, row) {bad[:4]}"


@pytest.mark.parametrize("family", A8.FAMILIES)
@pytest.mark.parametrize("seed", range(A8.N_SEEDS))
def test_8bit_random_launches_write_the_chosen_v_rows(family, seed):
    c = A8.case(family, seed)
    gap, chosen = A8.best_key_gaps(c)  # a check of the inputs, before any launch
    print(f"{family} seed {seed} {RL.describe(c.L)}: smallest lead of the best key {gap:.1f} log2 units")
    assert chosen and gap >= OH.MIN_GAP
    want = torch.as_tensor(c.expected()).to(c.dtype)
    for opts in A8.options(family, seed):
        out = _fresh(c)
        _launch(c, out, **({} if opts is None else dict(fp8_opts=opts)))
        torch.cuda.synchronize()
        _assert_bits(out, want, f"{family} seed {seed} {RL.describe(c.L)} fp8_opts {opts}")


@pytest.mark.parametrize("family", A8.FAMILIES)
@pytest.mark.parametrize("n_splits", (1, 3))
@pytest.mark.parametrize("dtype", A8.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_8bit_tied_keys_average_their_v_rows(family, dtype, n_splits):
    """A8.TIES: inside one 32-key group, across the 31 | 32 and the 63 | 64 edge, across a split boundary, into the partial last
    block.  The mx and i8 kernels weight a tied key of a block that is not the first of its split by a power of two only up to
    the rounding of its byte (their reference point moves by whole binades from the first block's maximum, not to the tied
    score), equally within a split and not across splits; their tie sets therefore start every split they touch in its
    first block.  The all-e4m3 kernel, whose reference point moves to the block maximum itself, also takes A8.TIES_FP8"""
    c, target = A8.tie_case(family, dtype, n_splits)
    sets = A8.tie_sets(family)
    gap, chosen = A8.best_key_gaps(c, tied=[sets[t] for t in target])
    assert chosen and gap >= OH.MIN_GAP
    want = c.expected(A8.mean_of_best)
    want16 = torch.as_tensor(want).to(dtype)
    assert (want16.double().numpy() == want).all()
    out = _fresh(c)
    _launch(c, out)
    torch.cuda.synchronize()
    got = out.cpu()
    bad = (got != want16).any(-1).nonzero().tolist()
    assert torch.equal(got, want16), f"{len(bad)} rows differ, first (head, row, tie) {[(h, r, sets[target[r]]) for h, r in bad[:4]]}"


@pytest.mark.parametrize("family", A8.FAMILIES)
@pytest.mark.parametrize("seed", range(A8.N_GRID_SEEDS))
def test_8bit_fused_grids_write_the_chosen_v_rows(family, seed, monkeypatch):
    """2 .. 6 random segments (A8.grid_cases, drawn like `_segments` of tests/test_hip_attention_random.py) over one set of k, v8, v_descale (and int8
    operands) as ONE fused grid through ops.attn_fwd_batch; every segment has the q of its own one-hot rows and its own output
    buffer, which equals its expected tensor bit for bit -- not only the stand-alone launch, with which it could share a slip"""
    from vorta_amd import ops
    cases = A8.grid_cases(family, seed)
    first, dtype = cases[0], cases[0].dtype
    for c in cases:
        gap, chosen = A8.best_key_gaps(c)
        assert chosen and gap >= OH.MIN_GAP, RL.describe(c.L)
    shared = _call(first, None)
    outs = [_fresh(c) for c in cases]
    calls = []
    for c, o in zip(cases, outs):
        kw = _call(c, o)
        kw.update({name: shared[name] for name in ("k", "v", "v_descale", "i8") if name in shared})  # ONE operand set
        calls.append(kw)
    single = []
    real_one = ops._launch_one
    monkeypatch.setattr(ops, "_launch_one", lambda a: (single.append(a), real_one(a)))
    ops.attn_fwd_batch(calls)
    torch.cuda.synchronize()
    assert not single, "every segment resolves to the 256-row pipelined kernel: the batch is one fused grid"
    for i, (c, o) in enumerate(zip(cases, outs)):
        _assert_bits(o, torch.as_tensor(c.expected()).to(dtype), f"{family} seed {seed} segment {i} of {len(cases)} {RL.describe(c.L)}")
