"""CPU-only: the rounding model of the attention forward and the float32 emulation of its loop (tests/_attn_fwd_model.py) are
checked themselves before any kernel is held to them (tests/test_hip_attention_fwd_structured.py,
tests/test_hip_attention_onehot.py).

  * without its roundings the model IS the attention forward: the restatement of tests/_attn_restate.py in float64, on the
    random launches of tests/test_host_backward_model.py, to 1e-12;
  * each of its three roundings shows by hand on three keys, and the row sum is NOT rounded;
  * the new input families are what they claim;
  * the cap: on every case the error of a plain float32 forward is at most a quarter of the model's, so the float32 term
    of the rule, 4 e_f32, adds at most one e_model.  A condition on the cases, not a measurement;
  * the rule can be met: the emulation stays at or under 0.9 of the bound on every row and every channel of every case,
    with c_row = c_ch = 3, the smaller of the two factors allowed.  A case that left 0.9 at factor 4 would be changed;
  * each gate can fail: three mutations of the EMULATION (never of the kernel) fail the gate they are meant for."""
import numpy as np
import pytest
import torch

import _attn_fwd_model as F
import _attn_onehot_inputs as OH
import _random_launch as RL
from _attn_restate import restate

IDS = dict(ids=F.dtype_name)


@pytest.mark.parametrize("seed", range(24))
def test_model_without_roundings_is_the_float64_restatement(seed):
    L = RL.draw(np.random.default_rng(3000 + seed), S_range=(64, 300), H_max=3)
    kw = RL.kwargs(L, "cpu")
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dtype = F.DTYPES[seed % 2]
    q, k, v = (torch.randn((L.H_buf, L.S, 128), generator=gen).to(dtype) for _ in range(3))
    want = restate(kw, q.double(), k.double(), v.double(), torch.full(q.shape, RL.SENTINEL, dtype=torch.float64))
    for variant in (0, 1):
        got = F.model_out(kw, q, k, v, dtype, round16=False, variant=variant, fill=RL.SENTINEL)
        e = float((got - want).abs().max())
        assert e <= 1e-12, f"seed {seed} {RL.describe(L)} variant {variant}: model without roundings is {e:.3e} from the restatement"
    valid, zero, dups = F.row_masks(kw, q.shape)
    assert torch.equal(valid | zero | dups, (want != RL.SENTINEL).any(-1)), "row_masks names the rows the launch writes"
    assert not want[zero].any()
    for h, rows, src in F.dup_pairs(kw, L.H_buf):
        assert torch.equal(want[h, rows], want[h, src])


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
def test_each_rounding_of_the_model_by_hand(dtype):
    """one query q = a e_0 and three keys k_j = j e_0, v_j = (1 + j eps) e_0 + [j = 2] sum_i (1 + i eps) e_i (i = 1 .. 100): with c = scale log2 e and
    qs = round16(a c) the scores are z_j = j qs, P_j = 2^(z_j - z_2), l = sum P (not rounded), p_j = round16(P_j),
    out_0 = round16(sum p_j (1 + j eps) / l), out_i = round16(p_2 (1 + i eps) / l).  a c, P_0, P_1 and the quotients are no 16-bit numbers,
    and l differs from the sum of the rounded p_j; variant 1 keeps qs = a c"""
    r16 = lambda x: float(torch.tensor(x, dtype=torch.float64).to(dtype))  # noqa: E731
    eps = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    a = 3.0 + 8 * eps
    q, k, v = (torch.zeros((1, 4, 128), dtype=dtype) for _ in range(3))
    q[0, 0, 0] = a
    for j in range(3):
        k[0, j, 0], v[0, j, 0] = j, 1 + j * eps
    for i in range(1, 101):
        v[0, 2, i] = 1 + i * eps
    assert float(q[0, 0, 0]) == a and float(v[0, 1, 0]) == 1 + eps
    c = F.LOG2E / 128 ** 0.5
    for rounded in (True, False):
        for variant in (0, 1):
            rr = r16 if rounded else (lambda x: x)
            qs = rr(a * c) if variant == 0 else a * c
            assert not rounded or r16(a * c) != a * c
            P = [2.0 ** ((j - 2) * qs) for j in range(3)]
            p = [rr(x) for x in P]
            l = sum(P)
            assert not rounded or (p[0] != P[0] and p[1] != P[1] and sum(p) != l and p[2] == 1.0)
            want0 = rr(sum(p[j] * (1 + j * eps) for j in range(3)) / l)
            want = lambda l_: [rr(p[2] * (1 + i * eps) / l_) for i in range(1, 101)]  # noqa: E731
            assert not rounded or want(l)[0] != p[2] / l
            got = F.model_out(dict(n_q=1, n_kv=3), q, k, v, dtype, round16=rounded, variant=variant, fill=RL.SENTINEL)
            assert abs(float(got[0, 0, 0]) - want0) <= 1e-15, (rounded, variant)
            assert np.abs(got[0, 0, 1:101].numpy() - np.array(want(l))).max() <= 1e-15, (rounded, variant)
            if rounded:  # a model that rounded l, or summed the rounded P, would give other numbers
                assert want(l) != want(r16(l)) and want(l) != want(sum(p))
            assert not got[0, 0, 101:].any() and (got[0, 1:] == RL.SENTINEL).all()


def test_the_new_families_are_what_they_claim():
    """staircase: over a contiguous key range the row maximum rises in at least 4 of the 6 blocks (by about 4 log2 units a
    block), the reference point of the loop is raised again and again, and between raises some block stands 4 to 6 above it
    (P up to 2^6); v_common: the mean of v is about 4"""
    for dtype in F.DTYPES:
        q, k, v = F.family("staircase", 1, F.S_VID, dtype)
        z = (q[0].double() @ k[0].double().t()) * F.LOG2E / 128 ** 0.5
        running = torch.cummax(z.reshape(F.S_VID, 6, 64).max(-1).values, 1).values
        rises = 1 + (running[:, 1:] > running[:, :-1]).sum(1)  # (the first block always sets it)
        assert rises.min() >= 4
        assert 3.5 < float((running[:, -1] - running[:, 0]).mean()) / 5 < 4.5
        info = {}
        F.emulate_out(dict(n_q=F.S_VID, n_kv=F.S_VID), q, k, v, dtype, info=info)
        print(f"staircase {F.dtype_name(dtype)}: {info}")
        assert info["raises"] >= 2 * F.S_VID and 4.0 <= info["max_lag"] <= 6.0
        info = {}
        F.emulate_out(dict(n_q=F.S_VID, n_kv=F.S_VID), *F.family("white", 1, F.S_VID, dtype), dtype, info=info)
        assert info["raises"] == 0  # (what the other families leave untouched)
        assert abs(float(F.family("v_common", 1, F.S_VID, dtype)[2].double().mean()) - 4) < 0.1


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
@pytest.mark.parametrize("fam,which", F.CASES)
def test_cap_float32_error_is_a_quarter_of_the_models(fam, which, dtype):
    c = F.case(fam, dtype, which)
    assert all(torch.isfinite(c[n]).all() for n in ("f64", "model", "f32", "emu"))
    assert c["valid"].any(), "the launch computes nothing"
    e_model, e_f32 = (F.fro((c[n] - c["f64"])[c["valid"]]) for n in ("model", "f32"))
    print(f"{fam} {F.dtype_name(dtype)} {which}: e_model {e_model:.3e} e_f32 {e_f32:.3e} e_f32 / e_model {e_f32 / e_model:.4f}")
    assert e_model > 0.0 and e_f32 <= e_model / 4
    for n in ("model", "f32", "emu"):  # what is exact in the kernel is exact in every reference
        assert not c[n][c["zero"]].any() and not c[n][~(c["valid"] | c["zero"] | c["dups"])].any()
        for h, rows, src in F.dup_pairs(c["kw"], c["H"]):
            assert torch.equal(c[n][h, rows], c[n][h, src])


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
@pytest.mark.parametrize("fam,which", F.CASES)
def test_the_emulation_meets_the_rule_with_margin(fam, which, dtype):
    """the emulation is the reference the margin is measured against; the kernel never is.  Largest ratios over all cases
    at factor 3: rows 0.89 (shift_up bf16 fused_table), channels 0.64 (late_key fp16 kv321), whole tensor 0.55"""
    c = F.case(fam, dtype, which)
    r = F.unit_ratios(c["emu"], c)
    worst = {unit: float(x.max()) for unit, x in r.items()}
    print(f"{fam} {F.dtype_name(dtype)} {which}: emulation / bound {worst}")
    assert F.C_ROW == 3.0 and F.C_CH == 3.0 and F.MARGIN == 0.9
    assert all(w <= F.MARGIN for w in worst.values()), worst


def test_forcing_one_split_on_the_gather_launches_changes_nothing():
    """both gather seeds carry n_splits = 1, so gather_a_s1 / gather_b_s1 are the launches gather_a / gather_b: the same
    keywords and the same references (what takes them through the split path is gather_*_s3)"""
    for name in ("gather_a", "gather_b"):
        kw, kw1 = F.launch(name)[2], F.launch(name + "_s1")[2]
        assert kw["n_splits"] == 1 and kw.keys() == kw1.keys()
        for key, val in kw.items():
            assert torch.equal(val, kw1[key]) if torch.is_tensor(val) else val == kw1[key], key
        assert F.launch(name + "_s3")[2]["n_splits"] == 3
        for dtype in F.DTYPES:
            assert torch.equal(F.case("white", dtype, name)["emu"], F.case("white", dtype, name + "_s1")["emu"])


def test_the_emulation_is_not_the_model():
    """they round P relative to different points, so they agree on most elements and not on all: the reason the rule compares
    errors and not outputs"""
    c = F.case("white", torch.bfloat16, "dense_256")
    same = float((c["emu"][c["valid"]] == c["model"][c["valid"]]).double().mean())
    print(f"emulation == model on {same:.2%} of the elements")
    assert 0.3 < same < 0.95


# ------------------------------------------------------------------------------------------------ each gate can fail
def _mutated(c, dtype, mutate):
    return F.emulate_out(c["kw"], c["q"], c["k"], c["v"], dtype, variant=c["variant"], mutate=mutate)


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
def test_mutation_one_dropped_key_fails_the_row_rule(dtype):
    """one key of one row masked out on white noise -- the key of MEDIAN probability of that row, about 1 / 650 -- fails the
    row's rule in both types and, in bf16, passes the whole-tensor rule"""
    c = F.case("white", dtype, "dense_256")
    pos = 200
    p = torch.softmax((c["q"][0, pos].double() @ c["k"][0].double().t()) / 128 ** 0.5, -1)
    key = int(p.argsort()[len(p) // 2])
    r = F.unit_ratios(_mutated(c, dtype, ("drop_key", 0, pos, key)), c)
    print(f"{F.dtype_name(dtype)}: key {key} of row {pos}, P {float(p[key]):.2e}: tensor {float(r['tensor']):.2f} row {float(r['row'][pos]):.2f}")
    assert float(r["row"][pos]) > 1.0 and int((r["row"] > 1.0).sum()) == 1
    if dtype == torch.bfloat16:  # (fp16's smaller roundings let even the whole tensor of 384 rows see it, at 1.5)
        assert float(r["tensor"]) <= 1.0


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
def test_mutation_one_scaled_channel_fails_the_channel_rule(dtype):
    """one channel of one 8-channel group 2 % off"""
    c = F.case("white", dtype, "dense_256")
    r = F.unit_ratios(_mutated(c, dtype, ("scale_channel", 77, 1.02)), c)
    print(f"{F.dtype_name(dtype)}: tensor {float(r['tensor']):.2f} rows {float(r['row'].max()):.2f} channel {float(r['channel'][0, 77]):.2f}")
    assert float(r["channel"][0, 77]) > 1.0 and int((r["channel"] > 1.0).sum()) == 1
    if dtype == torch.bfloat16:
        assert float(r["tensor"]) <= 1.0 and float(r["row"].max()) <= 1.0  # (only the channels see it)


def _onehot_launch():
    """a random launch of tests/test_hip_attention_onehot.py with groups that have key lists of their own"""
    for seed in range(32):
        L = RL.draw(np.random.default_rng(9300 + seed), S_range=(64, 600))
        if L.per_group and len(L.bounds) > 1 and len(L.live) and L.q_valid_eff > L.bounds[1][0] and L.n_splits > 1:
            return seed, L
    raise AssertionError("no such launch")


@pytest.mark.parametrize("dtype", F.DTYPES, **IDS)
def test_one_hot_inputs_are_exact_in_the_emulation_and_a_shifted_key_list_is_not(dtype):
    """the blocked float32 loop returns the chosen v rows with equal bits (every other probability and every rescale
    factor is exp2(<= -160) = 0); with the kv_rows of one group read one row further it does not"""
    seed, L = _onehot_launch()
    q, k, v, choice = OH.inputs(L, seed)
    gap, chosen = OH.best_key_gaps(L, q, k, choice, float(torch.tensor(5 * OH.SCALE * OH.LOG2E).to(dtype)) / 5)
    assert chosen and gap >= OH.MIN_GAP
    want = torch.as_tensor(RL.dense_reference(L, q, k, v, OH.pick_chosen))
    kw = dict(RL.kwargs(L, "cpu"), scale=OH.SCALE)
    qt, kt, vt = OH.tensors(dtype, "cpu", q, k, v)
    for variant in (0, 1):
        got = F.emulate_out(kw, qt, kt, vt, dtype, variant=variant, fill=RL.SENTINEL)
        assert torch.equal(got, want), (seed, variant)
    bad = F.emulate_out(kw, qt, kt, vt, dtype, fill=RL.SENTINEL, mutate=("shift_kv", 1))
    assert not torch.equal(bad, want)
    a, b = L.bounds[0]
    rows0 = L.written[a:b]
    assert all(torch.equal(bad[h, rows0], want[h, rows0]) for h in L.live)  # (the other groups are untouched)


def test_the_one_hot_inputs_reach_the_positions_they_must():
    for seed in range(32):
        L = RL.draw(np.random.default_rng(9300 + seed), S_range=(64, 600))
        choice = OH.inputs(L, seed)[3]
        forced = OH.forced_choices(L)
        assert 0 in forced and L.n_kv_eff - 1 in forced
        for a, b in L.bounds:
            if b - a >= len(forced):
                assert set(forced) <= set(choice[a:b].tolist())
        if max(b - a for a, b in L.bounds) >= 2:
            assert L.n_kv_eff - 1 in choice
