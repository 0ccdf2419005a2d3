"""CPU-only: the one-hot inputs of the 8-bit attention forwards (tests/_attn8_onehot_inputs.py) are what they claim, decided on
the launch emulator O.fp8_attn_launch alone before any kernel is held to them (tests/test_hip_attention_onehot_8bit.py).

Why the rows are exact, per family.  Every computed row has ONE key whose score leads every other by >= 160 log2 units
(asserted from the operands the kernel multiplies), so every other probability is exp2(<= -155): zero as a float32, zero as
an e4m3 byte (the smallest is 2^-9 under any scale the row can have).
  fp8  the scores q8 . k8 are integers (multiples of 2 A^2); the reference point moves to the block maximum itself, so the
       chosen key's probability is 2^p_bias: an exact byte.  Row sum 2^p_bias, 1.f / l_tot exact.
  mx   the scores are multiples of 20 (A8.SCALE); the reference point is the maximum of the first block of the split and
       moves by whole binades (the block exponent e), so the chosen key's probability is 2^(c - e) 2^e with whole c and e:
       an exact e4m3 byte under an exact mx scale code.  Row sum = that power of two, 1.f / l_tot exact.
  i8   the same to 1e-5 of a byte: the score unit u (q8 . k8) is a float32 product, 20 (1 +- 1e-7) per step, and the byte
       rint(8 c + 56 - 8 e) lands on the multiple of 8 that decodes to a power of two.
Then v_descale[head], a power of two per channel: exact.  Key splits: the split of the chosen key carries the largest
reference point and weight 1; every other weight is exp2(<= -155) = 0 in the kernels.  The emulator's float64 keeps those
remainders, 2^-150 of the sums they are added to -- below half a unit in the last place of every nonzero sum, which is why
no v byte is zero.

Tied keys average their v rows; see tests/_attn8_onehot_inputs.py for where that is exact in the mx and i8 kernels.

The tolerance tests and the last key: `test_what_the_tolerance_tests_see_of_a_dropped_key` drops the last effective key from
the Gaussian launches of tests/test_hip_attention_random.py::test_8bit_random_launches_vs_emulator, emulator on both
sides.  Measured (printed by the test, not asserted): `_check` passes 24 of the 48 cases -- the 24 that compute no row or
have a single key -- and 0 of the 24 that have a key to drop, every one on its max |d| bound: a Gaussian row has keys of
several times the mean probability, and the largest change over a launch's rows and channels leaves ATOL_SAME.  So that
slip is seen there too; what a tolerance cannot pin is WHICH key, row, scale or weight -- the slips (a), (c) - (f) below
shift values by amounts a flat softmax averages away, and the one-hot rows turn each of them into other bits.
"""
import numpy as np
import pytest
import torch

import _attn8_onehot_inputs as A8
import _attn_onehot_inputs as OH
import _random_launch as RL
from oracle import vorta_oracle as O

CASES = [(f, s) for f in A8.FAMILIES for s in range(A8.N_SEEDS)]


def _emulate_all(c, opts=None):
    L = c.L
    out, amb = np.full((L.H_buf, L.S, 128), RL.SENTINEL), np.zeros((L.H_buf, L.S))
    for h in L.live:
        c.emulate(h, out[h], amb[h], opts)
    return out, amb


def _assert_exact(c, want, opts, what, tied=None):
    gap, chosen = A8.best_key_gaps(c, tied)  # the precondition of every launch
    assert chosen and gap >= OH.MIN_GAP, (what, gap, chosen)
    out, amb = _emulate_all(c, opts)
    assert (amb == 0).all(), f"{what} {opts}: {(amb != 0).sum()} rows with a probability or a reference point in doubt"
    bad = np.argwhere((out != want).any(-1)).tolist()
    assert not bad, f"{what} {opts} {RL.describe(c.L)}: {len(bad)} rows differ, first (head, row) {bad[:4]}"
    return out


@pytest.mark.parametrize("family,seed", CASES)
def test_the_emulator_writes_exactly_the_expected_rows(family, seed):
    """float64 `==` on the whole buffer -- the computed rows, zeros past q_valid, the sentinel on the rows the launch does not
    name -- with no row in doubt: the share of rows left out is 0"""
    c = A8.case(family, seed)
    want = c.expected()
    L = c.L
    for h in L.live:  # (the reference itself: zeros past q_valid, the sentinel elsewhere)
        past = L.written[L.q_valid_eff:]
        assert not want[h, past].any()
    named = np.zeros(L.S, dtype=bool)
    named[L.written] = True
    if L.dup is not None:
        named[L.dup[:L.n_dup_pos].ravel()] = True
    assert (want[:, ~named] == RL.SENTINEL).all() and (want[np.setdiff1d(np.arange(L.H_buf), L.live)] == RL.SENTINEL).all()
    for opts in A8.options(family, seed):
        if opts and "flags" in opts:
            continue  # (the VALU row sum adds the unrounded P: the same numbers here, and not what the emulator models)
        _assert_exact(c, want, opts, f"{family} seed {seed}")


@pytest.mark.parametrize("family", A8.FAMILIES)
@pytest.mark.parametrize("n_splits", (1, 3))
@pytest.mark.parametrize("dtype", A8.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_the_emulator_averages_tied_keys_exactly(family, dtype, n_splits):
    c, target = A8.tie_case(family, dtype, n_splits)
    sets = A8.tie_sets(family)
    want = c.expected(A8.mean_of_best)
    assert (want[0, :len(sets)] == np.stack([c.v_eff[0, list(t)].mean(0) for t in sets])).all()
    for dt in A8.DTYPES:
        assert (torch.as_tensor(want).to(dt).double().numpy() == want).all()
    _assert_exact(c, want, None, "ties", tied=[sets[t] for t in target])


@pytest.mark.parametrize("family", A8.FAMILIES)
@pytest.mark.parametrize("seed", range(A8.N_GRID_SEEDS))
def test_the_emulator_writes_exactly_the_expected_rows_of_every_grid_segment(family, seed):
    cases = A8.grid_cases(family, seed)
    assert 2 <= len(cases) <= 6 and all(c.v8 is cases[0].v8 and (c.k == cases[0].k).all() for c in cases)
    for i, c in enumerate(cases):
        _assert_exact(c, c.expected(), None, f"{family} grid {seed} segment {i}")


# --------------------------------------------------------------------------------------------------------- sensitivity
def _perturbations(c):
    """name -> (feature on, emulator keywords of live head h that restate a kernel slip)"""
    L = c.L
    kw = RL.emulator_kwargs(L)
    h = int(L.live[0])
    keys = np.atleast_2d(kw["kv_rows"] if kw["kv_rows"] is not None else L.kv_off + np.arange(L.n_kv))
    rolled = np.roll(keys, -1, axis=-1)
    want = c.expected()
    rows = want[h, L.written]
    # a launch that computes nothing, or whose rows are all one row (a single effective key), shows no slip of the tables
    computes = L.q_valid_eff > 0 and bool((rows != rows[0]).any())
    src = want[h, L.written[:L.n_dup_pos]]
    src_of_rolled = np.arange(L.S)
    src_of_rolled[np.roll(L.written, 1)] = L.written
    return h, want, {
        # (rolling a key list whose every entry is in effect permutes the keys of a softmax: no slip to see)
        "a: key list rolled by one": (computes and any(set(a[:L.n_kv_eff]) != set(b[:L.n_kv_eff]) for a, b in zip(keys, rolled)),
                                      dict(kv_rows=rolled if L.per_group else rolled[0], kv_row_offset=0)),
        "b: last effective key dropped": (computes and L.n_kv_eff > 1, dict(n_kv=L.n_kv_eff - 1)),
        "c: v_descale of the next head": (computes and L.H_buf > 1, dict(vd=c.vd[(h + 1) % L.H_buf].astype(np.float64))),
        "d: v_descale rolled by one channel": (L.q_valid_eff > 0, dict(vd=np.roll(c.vd[h], 1).astype(np.float64))),
        # (every position computes its own query and writes the row of its neighbour: q_rows rolled by one for the stores,
        # the loads left alone -- rolled for both, a launch only renames its positions)
        "e: q_rows rolled by one": (computes, dict(q_rows=np.roll(L.written, 1), q_row_offset=0, q_src=src_of_rolled)),
        "f: dup_rows sources rolled by one": (L.n_dup_pos > 1 and bool((src != src[0]).any()),
                                              dict(dup_rows=None if L.dup is None else np.roll(L.dup[:L.n_dup_pos], 1, axis=0))),
    }


@pytest.mark.parametrize("family,seed", CASES)
def test_each_slip_changes_bits_of_an_expected_row(family, seed):
    """what a kernel slip would write, restated on the emulator's call: on every seed where the feature is on, bits of at least one
    row of the first live head change, in the output dtype"""
    c = A8.case(family, seed)
    if len(c.L.live) == 0:
        return
    h, want, perturbed = _perturbations(c)
    want16 = torch.as_tensor(want[h]).to(c.dtype)
    for name, (on, over) in perturbed.items():
        if not on:
            continue
        out, amb = np.full((c.L.S, 128), RL.SENTINEL), np.zeros(c.L.S)
        c.emulate(h, out, amb, **over)
        assert not torch.equal(torch.as_tensor(out).to(c.dtype), want16), f"{family} seed {seed} {RL.describe(c.L)}: {name} went unseen"


def test_every_slip_is_tried_on_several_seeds():
    seen = {}
    for family, seed in CASES:
        c = A8.case(family, seed)
        if len(c.L.live):
            for name, (on, _) in _perturbations(c)[2].items():
                seen[family, name[0]] = seen.get((family, name[0]), 0) + int(on)
    print(seen)
    assert all(seen.get((f, n), 0) >= 2 for f in A8.FAMILIES for n in "abcdef"), seen


def test_the_random_launches_reach_every_feature():
    """what the 16 seeds of each family cover, among the launches that compute anything: every routing feature, and chosen keys
    (of computed positions) on each side of a split boundary and of a 32-key edge, and in the partial last block"""
    names = ("splits", "q_rows", "kv_rows", "q_block_table", "duplicates", "device lengths", "split boundary chosen",
             "32-key edge chosen", "partial block chosen")
    for family in A8.FAMILIES:
        seen = dict.fromkeys(names, 0)
        for seed in range(A8.N_SEEDS):
            c = A8.case(family, seed)
            L = c.L
            if len(L.live) == 0 or L.q_valid_eff == 0:
                continue
            picked = set(c.choice[:L.q_valid_eff].tolist())
            bps = -(-(-(-L.n_kv // OH.KVB)) // L.n_splits)
            whole = L.n_kv_eff // OH.KVB * OH.KVB
            for name, on in (("splits", L.n_splits > 1), ("q_rows", L.q_rows is not None), ("kv_rows", L.kv_rows is not None),
                             ("q_block_table", L.qtab is not None), ("duplicates", L.n_dup_pos > 0),
                             ("device lengths", L.n_kv_dev is not None or L.q_valid_dev is not None),
                             ("split boundary chosen", any({s * bps * OH.KVB - 1, s * bps * OH.KVB} <= picked for s in range(1, L.n_splits))),
                             ("32-key edge chosen", {31, 32} <= picked),
                             ("partial block chosen", whole < L.n_kv_eff and any(p >= whole for p in picked))):
                seen[name] += int(on)
        print(family, seen)
        assert all(n >= 2 for n in seen.values()), (family, [k for k, n in seen.items() if n < 2])


# ------------------------------------------------------------------------------------------ what the tolerance tests see
def _gaussian_case(family, seed):
    """the launch and the operands of tests/test_hip_attention_random.py::test_8bit_random_launches_vs_emulator, the
    conversions restated by the oracle (pinned to the kernels bit for bit by tests/test_hip_fp8.py and test_hip_i8.py);
    returns emulate(h, out, amb, **over), L, dtype, max |v v_descale|"""
    from _util import rounded
    rng = np.random.default_rng(7000 + 100 * ("16", "fp8", "mx", "i8").index(family) + seed)
    dtype = A8.DTYPES[seed % 2]
    L = RL.draw(rng, S_range=(64, 600), empty_tail=seed % 4 == 3)
    x = [rng.standard_normal((L.H_buf, L.S, 128)) for _ in range(3)]
    if family == "i8":
        x[0] = x[0] + 0.7 * rng.standard_normal((1, 1, 128))
    q, k, v = (rounded(a, dtype) for a in x)
    z = O.fp8_quantize_qkv(q, k, v)
    v8, vd = O.e4m3_decode(z["v8"]), z["v_descale"].astype(np.float64)
    kw = RL.emulator_kwargs(L)
    if family == "fp8":
        q8, k8 = O.e4m3_decode(z["q8"]), O.e4m3_decode(z["k8"])
        run = lambda h, out, amb, **o: O.fp8_attn_launch(q8[h], k8[h], v8[h], out, vd[h], ambiguous=amb, **dict(kw, **o))  # noqa: E731
    elif family == "mx":
        c0 = float(np.float32(128 ** -0.5) * np.float32(OH.LOG2E))
        qe = (torch.as_tensor(q).to(dtype).float() * c0).to(dtype).double().numpy()
        run = lambda h, out, amb, **o: O.fp8_attn_launch(qe[h], k[h], v8[h], out, vd[h], ambiguous=amb, p_mode="rne_mx",  # noqa: E731
                                                         defer=24.0, **dict(kw, **o))
    else:
        i8 = O.i8_quantize_k(q, k)
        hook = lambda h: (lambda qr, kr: O.i8_wave_operands(q[h][qr], i8["q_prep"][h], i8["k_head_scale"][h], i8["k8"][h][kr],  # noqa: E731
                                                            i8["k_bias"][h][kr], None))
        run = lambda h, out, amb, **o: O.fp8_attn_launch(None, None, v8[h], out, vd[h], ambiguous=amb, p_mode="mx", defer=24.0,  # noqa: E731
                                                         wave_operands=hook(h), **dict(kw, **o))
    return run, L, dtype, float(np.abs(v8 * vd[:, None, :]).max())


def test_what_the_tolerance_tests_see_of_a_dropped_key():
    """perturbation (b), the last effective key dropped, on the Gaussian operands of the 48 random launches of the tolerance
    test, emulator on both sides: how many cases its `_check` still passes.  A measurement (printed; the figure of the module
    docstring), not an assertion: the flat softmax of 64 .. 600 Gaussian keys hides one key inside ATOL_SAME"""
    from test_hip_fp8 import _check
    passed, tried, caught = [], 0, {}
    for family in A8.FAMILIES:
        for seed in range(16):
            run, L, dtype, vmax = _gaussian_case(family, seed)
            if len(L.live) == 0 or L.q_valid_eff == 0 or L.n_kv_eff < 2:
                passed.append((family, seed, "nothing to drop"))
                continue
            tried += 1
            ref, amb, out = np.full((L.H_buf, L.S, 128), RL.SENTINEL), np.zeros((L.H_buf, L.S)), np.full((L.H_buf, L.S, 128), RL.SENTINEL)
            for h in L.live:
                run(h, ref[h], amb[h])
                run(h, out[h], np.zeros(L.S), n_kv=L.n_kv_eff - 1)
            try:
                _check(torch.as_tensor(out).to(dtype), ref, dtype, amb, vmax)
                passed.append((family, seed, "unseen"))
            except AssertionError as e:
                why = str(e).split("=")[0]
                caught[why] = caught.get(why, 0) + 1
    unseen = [p for p in passed if p[2] == "unseen"]
    print(f"`_check` passes {len(passed)} of 48 Gaussian launches with the last effective key dropped: {len(unseen)} of the {tried} "
          f"that compute a row and have a key to drop {unseen}, and the {len(passed) - len(unseen)} that do not; it fails the others on {caught}")
