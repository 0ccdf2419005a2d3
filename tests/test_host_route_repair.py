"""CPU: `vorta.patch.repair_routes`, the host rule `ops.route_repair` (vorta_route_repair) must equal bit for bit: which heads,
as launched, are over a stated error on the sampled rows, and the routes without them.  Crafted records: a rel exactly on
the bound and one float32 ulp above it, NaN and inf, sq_ref == 0, heads no list names, heads whose launch is the reference,
every number of tiers and every exact tier; the invariants of the outputs; the refusals."""
import itertools
import math

import pytest
import torch

from vorta_amd.patch import repair_routes

NAN, INF = float("nan"), float("inf")
# rel = sqrt(sq_err / sq_ref) in float32: 0.75 exactly for (9, 16); the next float32 above 0.75 squared, times 16, rounds to a
# sq_err whose rel is that next float32 (checked below, not assumed)
ULP_ABOVE = float(torch.nextafter(torch.tensor(0.75), torch.tensor(1.0)))


def _sq_err_of(rel: float, sq_ref: float) -> float:
    """a float32 sq_err whose float32 rel against sq_ref is exactly `rel` (searched among the neighbours of rel^2 sq_ref)"""
    guess = torch.tensor(rel * rel * sq_ref, dtype=torch.float32)
    for _ in range(8):
        got = float(torch.sqrt(guess / torch.tensor(sq_ref, dtype=torch.float32)))
        if got == rel:
            return float(guess)
        guess = torch.nextafter(guess, torch.tensor(INF if got < rel else -INF))
    raise AssertionError(f"no float32 sq_err gives rel {rel} against {sq_ref}")


#          sq_ref  sq_err                      expert  what
CRAFTED = [(16.0, 9.0, 1),                     # 0: rel exactly ON the bound 0.75: kept
           (16.0, _sq_err_of(ULP_ABOVE, 16.0), 2),   # 1: one float32 ulp above the bound: repaired
           (1.0, NAN, 1),                      # 2: NaN record (a head the measurement left out): repaired
           (NAN, 1.0, 2),                      # 3: NaN reference: repaired
           (1.0, INF, 1),                      # 4: inf: repaired
           (0.0, 0.0, 2),                      # 5: sq_ref == 0 and sq_err == 0: rel 0, kept
           (0.0, 1.0, 1),                      # 6: sq_ref == 0 and sq_err > 0: inf, repaired
           (16.0, 100.0, -1),                  # 7: no list names the head: not checked, whatever the record
           (16.0, 1.0, 2),                     # 8: rel 0.25: kept
           (NAN, NAN, 0),                      # 9: full attention: in the exact tier not checked, even with a NaN record
           (16.0, 16.0, 0),                    # 10: full attention over the bound: repaired in an 8-bit tier, skipped in the exact one
           (16.0, 4.0, 0)]                     # 11: full attention within the bound (0.5)
SQ_REF = [c[0] for c in CRAFTED]
SQ_ERR = [c[1] for c in CRAFTED]
EXPERTS = [c[2] for c in CRAFTED]
H = len(CRAFTED)


def _check_invariants(got, experts_in, tiers_in, n_tiers, exact):
    experts, tiers = got.expert_of_head.tolist(), got.tier_of_head.tolist()
    state = got.state_of_head.tolist()
    n = len(experts)
    for t in range(n_tiers):
        for e in range(3):
            heads = [h for h in range(n) if experts[h] == e and tiers[h] == t]
            assert got.counts[t, e] == len(heads)
            assert got.lists[t, e].tolist() == heads + [-1] * (n - len(heads))  # ascending, then the filler
    named = sum(e >= 0 for e in experts_in)
    assert int(got.counts.sum()) == named == sum(e >= 0 for e in experts)  # the counts sum to the named heads
    repaired = [h for h in range(n) if state[h] == 2]
    assert got.repair_count == len(repaired) and got.repair_list.tolist() == repaired + [-1] * (n - len(repaired))
    for h in range(n):
        checked = experts_in[h] >= 0 and not (experts_in[h] == 0 and tiers_in[h] == exact)
        assert (state[h] != 0) == checked, h
        assert math.isnan(float(got.rel[h])) == (not checked or math.isnan(SQ_REF[h]) or math.isnan(SQ_ERR[h])), h
        if state[h] == 2:
            assert (experts[h], tiers[h]) == (0, exact)
        else:
            assert (experts[h], tiers[h]) == (experts_in[h], tiers_in[h])



def test_crafted_records_one_tier():
    got = repair_routes(EXPERTS, None, 1, 0, SQ_REF, SQ_ERR, 0.75)
    assert got.state_of_head.tolist() == [1, 2, 2, 2, 2, 1, 2, 0, 1, 0, 0, 0]
    assert got.expert_of_head.tolist() == [1, 0, 0, 0, 0, 2, 0, -1, 2, 0, 0, 0]
    assert got.tier_of_head.tolist() == [0] * H
    assert got.repair_list.tolist()[:got.repair_count] == [1, 2, 3, 4, 6] and got.repair_count == 5
    assert got.counts.tolist() == [[8, 1, 2]]
    rel = got.rel.tolist()
    assert rel[0] == 0.75 and rel[1] == ULP_ABOVE and rel[5] == 0.0 and rel[6] == INF and rel[4] == INF and rel[8] == 0.25
    assert all(math.isnan(rel[h]) for h in (2, 3, 7, 9, 10, 11))  # NaN records, and the heads that were not checked
    assert got.rel.dtype == torch.float32


def test_the_bound_is_compared_in_float32():
    # 0.75 + 1e-9 rounds to 0.75 in float32: head 1 (one ulp above 0.75) stays repaired, head 0 (on it) kept
    got = repair_routes(EXPERTS, None, 1, 0, SQ_REF, SQ_ERR, 0.75 + 1e-9)
    assert got.state_of_head.tolist()[:2] == [1, 2]
    got = repair_routes(EXPERTS, None, 1, 0, SQ_REF, SQ_ERR, ULP_ABOVE)
    assert got.state_of_head.tolist()[:2] == [1, 1]
    got = repair_routes(EXPERTS, None, 1, 0, SQ_REF, SQ_ERR, 0.7499999)
    assert got.state_of_head.tolist()[:2] == [2, 2]


@pytest.mark.parametrize("n_tiers", [1, 2, 3])
def test_every_tier_count_and_exact_tier(n_tiers):
    for exact in range(n_tiers):
        for shift in range(n_tiers):
            tiers = [(h + shift) % n_tiers for h in range(H)]
            got = repair_routes(EXPERTS, tiers if n_tiers > 1 else None, n_tiers, exact, SQ_REF, SQ_ERR, 0.75)
            _check_invariants(got, EXPERTS, tiers, n_tiers, exact)
            state = got.state_of_head.tolist()
            # full attention in an 8-bit tier over the bound (head 10) moves to the exact tier; in the exact tier it is skipped,
            # NaN record (head 9) or not; within the bound (head 11) it stays where it is
            assert state[10] == (0 if tiers[10] == exact else 2)
            assert state[9] == (0 if tiers[9] == exact else 2)
            assert state[11] == (0 if tiers[11] == exact else 1)
            assert got.tier_of_head[10] == exact and got.expert_of_head[10] == 0
            assert state[7] == 0 and got.expert_of_head[7] == -1


def test_all_repaired_none_repaired_and_idempotence():
    experts, tiers = [1, 2, 0, 2, 1], [0, 0, 0, 1, 1]
    ref, err = [16.0] * 5, [1.0, 4.0, 9.0, 16.0, 25.0]   # rel 0.25, 0.5, 0.75, 1, 1.25
    none = repair_routes(experts, tiers, 2, 1, ref, err, INF)
    assert none.repair_count == 0 and none.state_of_head.tolist() == [1] * 5 and none.repair_list.tolist() == [-1] * 5
    assert none.expert_of_head.tolist() == experts and none.tier_of_head.tolist() == tiers
    every = repair_routes(experts, tiers, 2, 1, ref, err, 0.0)
    assert every.repair_count == 5 and every.state_of_head.tolist() == [2] * 5
    assert every.expert_of_head.tolist() == [0] * 5 and every.tier_of_head.tolist() == [1] * 5
    assert every.counts.tolist() == [[0, 0, 0], [5, 0, 0]] and every.lists[1, 0].tolist() == [0, 1, 2, 3, 4]
    for bound in (0.0, 0.5, 0.75, 1.0, INF):
        for exact in (0, 1):
            first = repair_routes(experts, tiers, 2, exact, ref, err, bound)
            again = repair_routes(first.expert_of_head, first.tier_of_head, 2, exact, ref, err, bound)
            assert again.repair_count == 0 and 2 not in again.state_of_head.tolist(), (bound, exact)
            assert torch.equal(again.expert_of_head, first.expert_of_head) and torch.equal(again.tier_of_head, first.tier_of_head)
            assert torch.equal(again.lists, first.lists) and torch.equal(again.counts, first.counts)
    for tiers3 in itertools.product(range(3), repeat=3):
        first = repair_routes([0, 1, 2], list(tiers3), 3, 2, [1.0] * 3, [4.0, NAN, 0.0], 1.0)
        again = repair_routes(first.expert_of_head, first.tier_of_head, 3, 2, [1.0] * 3, [4.0, NAN, 0.0], 1.0)
        assert again.repair_count == 0


def test_rel_is_correctly_rounded_in_float32():
    """rel against the two operations in DOUBLE, each rounded to float32: for float32 operands a double quotient or root
    rounded once more is the correctly rounded float32 one (53 >= 2 * 24 + 2 bits), and Python's `/` and `math.sqrt` on
    doubles are correctly rounded -- so this reference owes nothing to a vectorised math library"""
    import struct
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]  # noqa: E731
    g = torch.Generator().manual_seed(7)
    n = 1024
    for scale in (1.0, 1e-3, 3e3):
        ref = (torch.rand(n, generator=g) * 3000 + 1e-3).float()
        err = (torch.rand(n, generator=g) * ref * scale).float()
        got = repair_routes([1] * n, None, 1, 0, ref, err, 1.0)
        want = [f32(math.sqrt(f32(e / r))) for e, r in zip(err.tolist(), ref.tolist())]
        assert got.rel.tolist() == want
        assert got.state_of_head.tolist() == [1 if w <= 1.0 else 2 for w in want]
        # a bound that IS a head's rel keeps that head
        on = repair_routes([1] * n, None, 1, 0, ref, err, want[17])
        assert on.state_of_head[17] == 1


def test_tensors_and_lists_give_the_same_tables():
    a = repair_routes(EXPERTS, None, 1, 0, SQ_REF, SQ_ERR, 0.75)
    b = repair_routes(torch.tensor(EXPERTS, dtype=torch.int32), torch.zeros(H, dtype=torch.int32), 1, 0,
                      torch.tensor(SQ_REF), torch.tensor(SQ_ERR), torch.tensor(0.75))
    for x, y in zip(a, b):
        assert x == y if isinstance(x, int) else torch.equal(x, y) or (x.is_floating_point() and torch.equal(x.isnan(), y.isnan()))


def test_refusals():
    ok = dict(expert_of_head=EXPERTS, tier_of_head=None, n_tiers=1, exact_tier=0, sq_ref=SQ_REF, sq_err=SQ_ERR, repair_above=0.5)
    for bad, match in [(dict(repair_above=-0.1), "repair_above"), (dict(repair_above=NAN), "repair_above"),
                       (dict(repair_above=None), "repair_above"), (dict(n_tiers=0), "n_tiers"), (dict(n_tiers=4), "n_tiers"),
                       (dict(exact_tier=1), "exact_tier"), (dict(exact_tier=-1), "exact_tier"),
                       (dict(n_tiers=2), "tier_of_head"), (dict(tier_of_head=[0] * (H - 1)), "tier_of_head"),
                       (dict(tier_of_head=[1] * H), "tier indices"), (dict(expert_of_head=[3] * H), "expert ids"),
                       (dict(expert_of_head=[-2] * H), "expert ids"), (dict(expert_of_head=[]), "1 to 1024"),
                       (dict(expert_of_head=[0] * 1025, sq_ref=[1.0] * 1025, sq_err=[1.0] * 1025), "1 to 1024"),
                       (dict(expert_of_head=[0.0] * H), "integer"), (dict(sq_ref=SQ_REF[:-1]), "sq_ref"),
                       (dict(sq_err=[SQ_ERR]), "sq_err")]:
        with pytest.raises(ValueError, match=match):
            repair_routes(**dict(ok, **bad))
    assert repair_routes(**dict(ok, repair_above=0.0)).repair_count == 7  # a bound of 0 is a bound: exact heads alone are kept
