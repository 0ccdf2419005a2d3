"""Host: the tables `routed.sampled_expert_fidelity` is launched with (`routed.sample_launch_plan`: position order, coreset windows,
sliding key-list classes and block tables) against a token-by-token restatement on the three geometries of the GPU tests; the
validation of `vorta.patch.fixed_routes`; `routes_from_fidelity` / `evaluate_routing` on a record of the new kind."""
import numpy as np
import pytest
import torch

from vorta_amd import _partial

WINDOW, GROUP = (3, 3, 3), (2, 3, 2)
GEOMETRIES = [((8, 6, 8), (2, 3, 4)), ((7, 9, 6), (2, 2, 4)), ((8, 12, 12), (2, 3, 4))]


def _restate(latent, tile, tokens, t_eff):
    """per sampled token, by loops: the first tile of its clamped window per dimension (the key list), the list's video keys
    counted tile by tile, and the coreset window"""
    nt = [-(-l // t) for l, t in zip(latent, tile)]
    lists, lengths, wins = [], [], []
    ng = [l // g for l, g in zip(latent, GROUP)]
    for tok in tokens:
        c = (tok // (latent[1] * latent[2]), (tok // latent[2]) % latent[1], tok % latent[2])
        first, keys = [], 1
        for d in range(3):
            half = WINDOW[d] // 2
            centre = min(max(c[d] // tile[d], half), nt[d] - 1 - half)
            f = max(centre - half, 0)
            cnt = min(nt[d], 2 * half + 1)
            keys *= sum(min(tile[d], latent[d] - i * tile[d]) for i in range(f, f + cnt))
            first.append(f)
        lists.append(tuple(first))
        lengths.append(keys + t_eff)
        inside = all(c[d] < ng[d] * GROUP[d] for d in range(3))
        wins.append(((c[0] // GROUP[0]) * ng[1] + c[1] // GROUP[1]) * ng[2] + c[2] // GROUP[2] if inside else -1)
    return lists, lengths, wins


@pytest.mark.parametrize("t_eff", [0, 11])
@pytest.mark.parametrize("latent,tile", GEOMETRIES)
def test_plan_against_a_token_by_token_restatement(latent, tile, t_eff):
    from vorta_amd.routed import sample_launch_plan, sample_rows
    S = latent[0] * latent[1] * latent[2]
    every = _restate(latent, tile, range(S), t_eff)
    all_lengths = sorted(set(every[1]), reverse=True)
    assert all_lengths == [n + t_eff for n in _partial.sliding_key_counts(latent, tile, WINDOW)]
    lists_of = {n: sorted({l for l, m in zip(every[0], every[1]) if m == n}) for n in all_lengths}
    for n, block_rows in ((S, 256), (96, 256), (S, 128), (0, 256)):
        tokens = sample_rows(S, n, 3).numpy().astype(np.int64)
        plan = sample_launch_plan(latent, tile, WINDOW, GROUP, tokens, t_eff, block_rows)
        lists, lengths, wins = _restate(latent, tile, tokens.tolist(), t_eff)
        want = sorted(range(n), key=lambda p: (-lengths[p], lists[p], p))
        assert plan["order"].tolist() == want and plan["order"].dtype == np.int64
        assert plan["win"].tolist() == [wins[p] for p in want] and plan["win"].dtype == np.int32
        at = 0
        for c in plan["classes"]:
            n_kv = c["n_kv"]
            mine = [p for p in want if lengths[p] == n_kv]
            assert mine and (c["start"], c["count"]) == (at, len(mine)) and c["index"] == all_lengths.index(n_kv)
            assert c["n_lists"] == len(lists_of[n_kv])
            table, covered = c["table"], 0
            assert table.dtype == np.int32 and table.shape[1] == 3
            for g, p0, p1 in table.tolist():
                assert p0 == covered and 0 < p1 - p0 <= block_rows and p1 <= len(mine)  # the blocks tile the class in order
                assert all(lists[mine[p]] == lists_of[n_kv][g] for p in range(p0, p1)), "a block holds one key list's rows"
                covered = p1
            assert covered == len(mine)
            # a block ends where its list ends or at block_rows: no list is cut into more blocks than it needs
            per_list = {g: sum(1 for p in mine if lists[p] == lists_of[n_kv][g]) for g in {r[0] for r in table.tolist()}}
            assert len(table) == sum(-(-m // block_rows) for m in per_list.values())
            at += len(mine)
        assert at == n and [c["n_kv"] for c in plan["classes"]] == sorted({lengths[p] for p in want}, reverse=True)
    if latent == (7, 9, 6):
        assert len(all_lengths) == 3 and -1 in every[2]  # the partial case: three launches, remainder tokens
    else:
        assert len(all_lengths) == 1 and -1 not in every[2]


def test_the_plan_agrees_with_the_librarys_list_lengths():
    """the host plan counts a list's keys itself; the partial tables count them in the library (vorta_sta_partial_sizes)"""
    from vorta_amd import ops
    from vorta_amd.routed import sample_launch_plan
    latent, tile = GEOMETRIES[1]
    S = latent[0] * latent[1] * latent[2]
    _, n_lists, _, lens = ops.sta_partial_sizes(latent, tile, WINDOW, 11)
    plan = sample_launch_plan(latent, tile, WINDOW, GROUP, np.arange(S), 11)
    used = sorted({n for n in lens}, reverse=True)
    assert [c["n_kv"] for c in plan["classes"]] == used  # (n = S: every class holds a position)
    for c in plan["classes"]:
        assert c["n_lists"] <= sum(1 for n in lens if n == c["n_kv"])


class _Plan:
    heads = 4

    def __len__(self):
        return 3


def _patched_stub():
    from vorta_amd.patch._engine import StepContext
    model = torch.nn.Linear(2, 2)
    model._vorta_ctx = StepContext(plan=_Plan())
    return model


def test_fixed_routes_validates_shape_and_ids():
    from vorta.patch import fixed_routes
    model = _patched_stub()
    good = torch.tensor([[0, 1, 2, 0], [2, 2, 1, 1], [0, 0, 0, 0]])
    with fixed_routes(model, good):
        assert model._vorta_ctx.fixed_routes == good.tolist()
        with fixed_routes(model, good.tolist()):  # nests, and takes a list of lists
            pass
        assert model._vorta_ctx.fixed_routes == good.tolist()
    assert model._vorta_ctx.fixed_routes is None
    for bad in (good[:2], good[:, :3], good.flatten(), good + 1, good - 1, good.float(), good.bool()):
        with pytest.raises(ValueError, match="fixed_routes"):
            with fixed_routes(model, bad):
                pass
    assert model._vorta_ctx.fixed_routes is None
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        with fixed_routes(torch.nn.Linear(2, 2), good):
            pass
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        from vorta.patch import sampled_expert_fidelity
        with sampled_expert_fidelity(torch.nn.Linear(2, 2)):
            pass
    with pytest.raises(RuntimeError, match="sampled_expert_fidelity"):
        from vorta.patch import sampled_expert_fidelity_of
        sampled_expert_fidelity_of(model)


def test_routes_and_evaluation_take_the_new_record():
    """a stacked record as `sampled_expert_fidelity_of` returns it: (L, H) references, (L, H, 3) errors with the routed output in
    column 2"""
    from vorta.patch import evaluate_routing, routes_from_fidelity
    from vorta.patch.fidelity import stack_fidelity
    from vorta_amd.ops import ExpertFidelity
    rel = torch.tensor([[[0.20, 0.03, 0.03], [0.04, 0.30, 0.04], [0.40, 0.50, 0.0], [0.01, 0.02, 0.02]],
                        [[0.06, 0.05, 0.05], [0.05, 0.06, 0.05], [0.9, 0.9, 0.0], [float("nan"), 0.01, 0.01]]])
    ref = torch.full((2, 4), 4.0)
    layers = [ExpertFidelity(ref[l], ref[l].sqrt(), (rel[l] ** 2) * 4.0, rel[l], ref[l], 64 * 128) for l in range(2)]
    fid = stack_fidelity(layers)
    assert torch.allclose(fid.rel_error(), rel, equal_nan=True)
    table = routes_from_fidelity(fid, 0.05)
    assert table.tolist() == [[2, 1, 0, 2], [2, 1, 0, 2]]
    geometry = dict(latent=(8, 6, 8), tile=(2, 3, 4), window=WINDOW, group=GROUP, rate=0.5)
    r = evaluate_routing(table, fid, geometry)
    assert torch.allclose(r["worst_rel_error"], torch.tensor([0.04, 0.05])) and r["experts"].tolist() == table.tolist()
    assert bool((r["flops_share"] < 1).all())
