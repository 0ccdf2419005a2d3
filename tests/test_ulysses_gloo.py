"""world_size > 1 on CPU (gloo): the Ulysses collectives against the golden maps captured from the reference,
and the zero-copy layout engine (index maps, head placement, round trip).  No GPU, no HIP."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import vorta_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _comm_worker(rank, world, port, ret):
    _init(rank, world, port)
    from vorta_amd.ulysses import SP_STATE, all_gather, all_to_all_4D, shrink_dim
    SP_STATE.setup_sp_group(world)
    g = np.load(os.path.join(GOLDEN, "g9_ulysses_maps.npz"))
    x = torch.from_numpy(g[f"P{world}_r{rank}_x"])
    y = all_to_all_4D(x, scatter_idx=1, gather_idx=2)
    z = all_to_all_4D(y, scatter_idx=2, gather_idx=1)
    t = torch.from_numpy(g[f"P{world}_r{rank}_t"])
    t_loc = shrink_dim(t, dim=1).contiguous()
    t_all = all_gather(t_loc, dim=1)
    ok = (np.array_equal(y.numpy(), g[f"P{world}_r{rank}_y"]) and np.array_equal(z.numpy(), g[f"P{world}_r{rank}_z"])
          and np.array_equal(t_loc.numpy(), g[f"P{world}_r{rank}_t_loc"])
          and np.array_equal(t_all.numpy(), g[f"P{world}_r{rank}_t_all"]))
    # batch > 1 goes through the packing copy
    xb = torch.cat([x, x + 0.5], dim=0)
    yb = all_to_all_4D(xb, 1, 2)
    ok = ok and torch.equal(yb[0], y[0]) and torch.equal(yb[1], y[0] + 0.5) and torch.equal(all_to_all_4D(yb, 2, 1), xb)
    try:
        all_to_all_4D(x, 3, 1)
        ok = False
    except RuntimeError:
        pass
    ret[rank] = bool(ok)
    dist.barrier()
    SP_STATE.cleanup()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_collectives_match_reference_maps(world):
    ret = mp.Manager().dict()
    mp.spawn(_comm_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert all(ret[r] for r in range(world)), dict(ret)


def _tag(h, s, d):
    return h * 100000.0 + s + d * 0.125


def _engine_worker(rank, world, port, ret):
    _init(rank, world, port)
    from vorta_amd.ulysses import UlyssesLayout, balanced_head_order
    H, S, T, D, P = max(8, 2 * world), 24 * world, 5, 4, world
    lay = UlyssesLayout(H, S, T, D, P, rank, "cpu", torch.float32)
    Hl, Sl = lay.Hl, lay.Sl
    experts = ([0, 2, 1, 1, 0, 2, 2, 1] if world == 2 else [0, 1, 2, 0, 1, 2, 1, 1]) * (H // 8)
    order = balanced_head_order(experts, [7.0, 2.0, 1.0], P)
    hs = torch.arange(H).view(H, 1, 1)
    ss = (torch.arange(Sl) + rank * Sl).view(1, Sl, 1)
    dd = torch.arange(D).view(1, 1, D)
    shards = [_tag(hs, ss, dd) + 1e7 * t for t in range(3)]  # q,k,v tagged by (head, global token, d)
    texts = [_tag(hs, torch.arange(T).view(1, T, 1) + 90000, dd) + 1e7 * t for t in range(3)]
    bufs = [lay.new_buffer().fill_(-1) for _ in range(3)]
    lay.scatter_heads(shards, bufs, order, texts)
    ok = True
    rm = lay.row_map.long()
    for t in range(3):
        hv = lay.head_view(bufs[t])
        for i in range(Hl):
            h = order[rank * Hl + i]
            got = hv[i][rm]  # (S+T, D) in token order
            want = torch.cat([_tag(torch.tensor(float(h)), torch.arange(S).view(S, 1), dd[0]),
                              _tag(torch.tensor(float(h)), torch.arange(T).view(T, 1) + 90000, dd[0])]) + 1e7 * t
            ok = ok and torch.equal(got, want)
    # identity "attention": O = Q, then travel back
    out_shard = torch.full((H, Sl, D), -2.0)
    out_text = torch.full((H, T, D), -2.0)
    lay.gather_heads(bufs[0], out_shard, order, out_text)
    ok = ok and torch.equal(out_shard, shards[0]) and torch.equal(out_text, texts[0])
    keep = lay.head_view(bufs[0]).clone().numpy()
    # other transport shapes of the same exchange: heads of every peer already consecutive (sent straight from
    # the shard, no staging pass), and strided shards / outputs (the projection's (Sl, H*D) buffer seen per head)
    for order2, strided in ((list(range(H)), False), (order, True), (list(range(H)), True)):
        sh2 = [x.transpose(0, 1).contiguous().transpose(0, 1) for x in shards] if strided else shards
        assert sh2[0].is_contiguous() != strided
        b2 = [lay.new_buffer().fill_(-1) for _ in range(3)]
        lay.scatter_heads(sh2, b2, order2, texts)
        for t in range(3):
            hv = lay.head_view(b2[t])
            for i in range(Hl):
                h = order2[rank * Hl + i]
                want = torch.cat([_tag(torch.tensor(float(h)), torch.arange(S).view(S, 1), dd[0]),
                                  _tag(torch.tensor(float(h)), torch.arange(T).view(T, 1) + 90000, dd[0])]) + 1e7 * t
                ok = ok and torch.equal(hv[i][rm], want)
        o2 = torch.full((Sl, H, D), -2.0).transpose(0, 1) if strided else torch.full((H, Sl, D), -2.0)
        t2 = torch.full((H, T, D), -2.0)
        lay.gather_heads(b2[0], o2, order2, t2)
        ok = ok and torch.equal(o2, shards[0]) and torch.equal(t2, texts[0])
    # the overlapped form: two slot groups, identity "attention" per group (O = Q on that group's slots only)
    from vorta_amd.ulysses import exchange_and_attend, slot_groups
    order3 = balanced_head_order(experts, [7.0, 2.0, 1.0], P, groups=2)
    assert sorted(order3) == list(range(H))
    b3 = [lay.new_buffer().fill_(-1) for _ in range(4)]
    seen = []

    sgs = lay.grouping(2)[0]  # a slot group is a receive layout of its own inside the buffers

    def attend(g0, g1, gi):
        seen.append((g0, g1, gi))
        sg = sgs[gi]
        for t in range(3):  # every slot of the group holds its head's whole sequence + text, in token order, through ITS row map
            hv, rmg = sg.head_view(b3[t]), sg.lay.row_map.long()
            for i in range(g0, g1):
                h = order3[rank * Hl + i]
                want = torch.cat([_tag(torch.tensor(float(h)), torch.arange(S).view(S, 1), dd[0]),
                                  _tag(torch.tensor(float(h)), torch.arange(T).view(T, 1) + 90000, dd[0])]) + 1e7 * t
                assert torch.equal(hv[i - g0][rmg], want), (t, i)
        sg.head_view(b3[3]).copy_(sg.head_view(b3[0]))

    o3, t3 = torch.full((H, Sl, D), -2.0), torch.full((H, T, D), -2.0)
    exchange_and_attend(lay, shards, b3, order3, texts, slot_groups(Hl, 2), attend, o3, t3)
    ok = ok and seen == [(0, Hl // 2, 0), (Hl // 2, Hl, 1)] and torch.equal(o3, shards[0]) and torch.equal(t3, texts[0])
    # every group's exchange is ONE all_to_all_single per tensor (the reference's collective, vorta/ulysses/utils.py:48,80):
    # 3 tensors in + 1 back, per group -- counted on the wire API
    calls = []
    real = dist.all_to_all_single
    dist.all_to_all_single = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        exchange_and_attend(lay, shards, b3, order3, texts, slot_groups(Hl, 2), attend, o3, t3)
    finally:
        dist.all_to_all_single = real
    ok = ok and len(calls) == 8 and not hasattr(lay, "_start")
    # the same layout expressed with the oracle's reference maps: seq->head of the head-permuted shard
    ret[rank] = (bool(ok), order, shards[0].numpy(), keep, rm.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_zero_copy_layout_round_trip(world):
    ret = mp.Manager().dict()
    mp.spawn(_engine_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert all(ret[r][0] for r in range(world))
    # cross-check against the reference's all_to_all_4D semantics (oracle): after permuting heads by the
    # placement order, rank r must hold exactly what the reference's reshard would give it
    order = ret[0][1]
    P = world
    shards = [ret[r][2][None][:, order] for r in range(P)]  # (1,H,Sl,D) with heads in placement order
    ref = O.ulysses_seq_to_head(shards)  # rank r: (1, Hl, S, D)
    for r in range(P):
        hv, rm = ret[r][3], ret[r][4]
        S = ref[r].shape[2]
        for i in range(ref[r].shape[1]):
            assert np.array_equal(hv[i][rm[:S]], ref[r][0, i])


def _uneven_worker(rank, world, port, ret):
    """ranks holding DIFFERENT numbers of heads (balanced_placement): every head's full sequence lands on its rank, the
    identity attention travels back, one group and two slot groups (per-rank split sizes of the all_to_all_single)"""
    _init(rank, world, port)
    from vorta_amd.ulysses import UlyssesLayout, balanced_placement, exchange_and_attend, slot_groups
    P = world
    H, S, T, D = 3 * world + 1, 24 * world, 5, 4
    experts = ([0, 2, 2, 1, 2, 2, 1] * H)[:H]
    cost = [7.0, 2.0, 1.0]
    ok = True
    hs = torch.arange(H).view(H, 1, 1)
    dd = torch.arange(D).view(1, 1, D)
    for groups in (1, 2):
        order, counts = balanced_placement(experts, cost, P, groups)
        ok = ok and sorted(order) == list(range(H)) and sum(counts) == H and min(counts) >= 1 and len(set(counts)) > 1
        lay = UlyssesLayout(H, S, T, D, P, rank, "cpu", torch.float32, counts=counts)
        Hl, Sl = lay.Hl, lay.Sl
        ok = ok and Hl == counts[rank] and not lay.even
        ss = (torch.arange(Sl) + rank * Sl).view(1, Sl, 1)
        shards = [_tag(hs, ss, dd) + 1e7 * t for t in range(3)]
        texts = [_tag(hs, torch.arange(T).view(1, T, 1) + 90000, dd) + 1e7 * t for t in range(3)]
        rm = lay.row_map.long()
        bufs = [lay.new_buffer().fill_(-1) for _ in range(4)]
        sg = slot_groups(Hl, min(groups, min(counts)))
        sgs = lay.grouping(len(sg))[0]
        seen = []

        def attend(g0, g1, gi):
            seen.append((g0, g1))
            grp = sgs[gi]
            rmg = grp.lay.row_map.long()
            for t in range(3):  # every local head slot holds its head's whole sequence + text, in token order
                hv = grp.head_view(bufs[t])
                for i in range(g0, g1):
                    h = order[lay.starts[rank] + i]
                    want = torch.cat([_tag(torch.tensor(float(h)), torch.arange(S).view(S, 1), dd[0]),
                                      _tag(torch.tensor(float(h)), torch.arange(T).view(T, 1) + 90000, dd[0])]) + 1e7 * t
                    assert torch.equal(hv[i - g0][rmg], want), (groups, t, i)
            grp.head_view(bufs[3]).copy_(grp.head_view(bufs[0]))

        o, tx = torch.full((H, Sl, D), -2.0), torch.full((H, T, D), -2.0)
        exchange_and_attend(lay, shards, bufs, order, texts, sg, attend, o, tx)
        ok = ok and seen == sg and torch.equal(o, shards[0]) and torch.equal(tx, texts[0])
    ret[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


def _selfcheck_worker(rank, world, port, ret):
    """exchange_selfcheck (bench.py's N > 1 pre-flight): integer-tagged q,k,v through the layout's own exchange, exact on every
    rank; a rank whose copy of the head order differs must fail it everywhere"""
    _init(rank, world, port)
    from vorta_amd.ulysses import (UlyssesLayout, balanced_head_order, balanced_placement, exchange_selfcheck, slot_groups)
    P = world
    S, T, D = 40 * world, 6, 8
    res = {}
    for H, uneven in ((3 * world, False), (5 * world + 1, True)):  # (3 and >= 3 slots per rank: up to three slot groups)
        experts = ([0, 2, 2, 1, 2, 2, 1] * H)[:H]
        cost = [7.0, 2.0, 1.0]
        for groups in (1, 2, 3):
            if uneven:
                order, counts = balanced_placement(experts, cost, P, groups)
            else:
                order, counts = balanced_head_order(experts, cost, P, groups), None
            lay = UlyssesLayout(H, S, T, D, P, rank, "cpu", torch.bfloat16, counts=counts)
            sg = slot_groups(lay.Hl, min(groups, min(lay.counts)))
            for brk in (False, True):
                bufs = [lay.new_buffer() for _ in range(4)]
                r = exchange_selfcheck(lay, order, sg, bufs, break_order=brk)
                res[(H, groups, brk)] = (r["ok"], r["bytes"] > 0, r["ms"] >= 0)
    ret[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def _split_worker(rank, world, port, ret):
    """heads split by QUERY RANGE over two ranks (split_placement): both ranks receive the head, each returns its range
    (zeros elsewhere: the identity attention of exchange_selfcheck honours the range), and every token shard must come
    back whole -- one group and two slot groups; a wrong range table must fail"""
    _init(rank, world, port)
    from vorta_amd.ulysses import UlyssesLayout, exchange_selfcheck, slot_groups, split_placement, placement_loads
    P = world
    S, D = 512 * world, 8
    H = 2 * world + 1
    experts = ([0, 0, 0, 2, 1, 2, 2, 1, 2] * H)[:H]  # three full-attention heads: whole heads cannot balance 2 or 4 ranks
    cost = [9.0, 2.0, 1.0]
    res = {}
    for gk, T in ((1, 0), (2, 0), (11, 6), (12, 6)):  # 1x: six text rows behind every head's video rows (owner: the last part)
        groups = gk % 10
        order, counts, parts = split_placement(experts, cost, P, S, groups, align=32, tol=0.005)
        n_extra = sum(counts) - H
        loads = placement_loads(experts, cost, order, counts, parts, S)
        res[("extra", gk)] = n_extra
        res[("ratio", gk)] = max(loads) * P / sum(loads)
        lay = UlyssesLayout(H, S, T, D, P, rank, "cpu", torch.bfloat16, counts=counts)
        sg = slot_groups(lay.Hl, min(groups, min(lay.counts)))
        bufs = [lay.new_buffer() for _ in range(4)]
        r = exchange_selfcheck(lay, order, sg, bufs, parts=parts)
        res[(gk, "ok")] = r["ok"]
        # the same exchange told that every slot is whole must lose the rows only the other part returned
        wrong = [None if p is None else (min(p[0] + 32, p[1] - 32), p[1]) for p in parts]
        bufs = [lay.new_buffer() for _ in range(4)]
        r = exchange_selfcheck(lay, order, sg, bufs, parts=wrong)
        res[(gk, "wrong ranges")] = r["ok"]
    ret[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_heads_split_by_query_range_round_trip(world):
    ret = mp.Manager().dict()
    mp.spawn(_split_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    for r in range(world):
        res = ret[r]
        for groups in (1, 2, 11, 12):  # (1x: with 6 text rows per head)
            assert res[("extra", groups)] >= 1, res            # the mix needs at least one split
            assert res[("ratio", groups)] <= 1.03, res  # (32-token steps of a 512-token shard are coarse)
            assert res[(groups, "ok")] is True, (r, groups)
            assert res[(groups, "wrong ranges")] is False, (r, groups)


def test_split_placement_reaches_one_percent_on_wan14b_at_eight_ranks():
    """Wan-14B-81f, 40 heads on 8 ranks: whole heads leave the heaviest rank at 1.037 of the mean, query
    ranges of full-attention heads bring every layer to <= 1.01 (costs: algorithmic FLOPs per head as bench.py counts them)"""
    from vorta_amd.ulysses import balanced_placement, placement_loads, split_placement
    S = 21 * 45 * 80
    cost = [2926264320000.0, 731566080000.0, 526727577600.0]  # full / coreset / sliding-tile, Wan-14B-81f
    for n0, n1, n2 in ((14, 13, 13), (7, 13, 20)):  # bench.py's uniform and sparse-heavy mixes at 40 heads
        for layer in range(40):
            e = np.random.default_rng(1234 + layer).permutation([0] * n0 + [1] * n1 + [2] * n2)
            o, c = balanced_placement(e, cost, 8)
            whole = placement_loads(e, cost, o, c)
            order, counts, parts = split_placement(e, cost, 8, S)
            loads = placement_loads(e, cost, order, counts, parts, S)
            assert abs(sum(loads) - sum(whole)) < 1e-6 * sum(whole)          # nothing computed twice
            assert max(loads) * 8 / sum(loads) <= 1.01 < max(whole) * 8 / sum(whole)
            st = np.cumsum([0] + counts)
            for j in range(8):  # at most two partial heads per rank (segments of its fused launch), full-attention heads only
                mine = [i for i in range(st[j], st[j + 1]) if parts[i] is not None]
                assert len(mine) <= 2 and all(e[order[i]] == 0 for i in mine)
            for h in set(order):  # the parts of a head tile its tokens exactly once
                rng = sorted(parts[i] or (0, S) for i in range(len(order)) if order[i] == h)
                assert rng[0][0] == 0 and rng[-1][1] == S and all(a[1] == b[0] for a, b in zip(rng, rng[1:]))


def _default_placement_worker(rank, world, port, ret):
    """no VORTA_SP_* in the environment: the processors' placement rule (vorta_amd/attention/_sp.py place_heads) takes `even`
    where P divides the heads and `uneven` where it does not, and the placement it returns passes the exchange's self-check"""
    for k in [k for k in os.environ if k.startswith("VORTA_SP_")]:
        del os.environ[k]
    _init(rank, world, port)
    import vorta_amd.attention._sp as sp
    from vorta_amd.ulysses import UlyssesLayout, exchange_selfcheck, slot_groups
    P, S, T, D = world, 40 * world, 6, 8
    res = {"default": sp.SP_PLACEMENT}
    for H in (2 * world, 3 * world + 1):
        experts = ([0, 2, 2, 1, 2, 2, 1] * H)[:H]
        placement, order, counts, parts = sp.place_heads(experts, [7.0, 2.0, 1.0], P, S)
        lay = UlyssesLayout(H, S, T, D, P, rank, "cpu", torch.bfloat16, counts=counts)
        r = exchange_selfcheck(lay, order, slot_groups(lay.Hl, 1), [lay.new_buffer() for _ in range(4)])
        res[H] = (placement, list(counts), parts is None, r["ok"])
    ret[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_default_placement_is_auto_even_when_ranks_divide_heads(world):
    ret = mp.Manager().dict()
    mp.spawn(_default_placement_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    for r in range(world):
        res = ret[r]
        assert res["default"] == "auto"
        placement, counts, whole, ok = res[2 * world]
        assert placement == "even" and counts == [2] * world and whole and ok, (r, res)
        placement, counts, whole, ok = res[3 * world + 1]
        assert placement == "uneven" and sum(counts) == 3 * world + 1 and whole and ok, (r, res)


def test_placement_rule_names():
    from vorta_amd.ulysses.state import resolve_placement
    assert resolve_placement("auto", 24, 8) == "even" and resolve_placement("auto", 12, 8) == "uneven"
    assert resolve_placement("uneven", 24, 8) == "uneven" and resolve_placement("split", 40, 8) == "split"
    with pytest.raises(ValueError):
        resolve_placement("even", 12, 8)
    with pytest.raises(ValueError):
        resolve_placement("balanced", 24, 8)


def test_split_placement_boundaries_are_workgroup_aligned_at_production_sizes():
    """boundaries are counted from the front in `align` steps, so every boundary except S itself is a multiple
    of `align` also where S is not (32 760 = 24 mod 32, 75 600 = 16 mod 32); parts tile each head exactly once"""
    from vorta_amd.ulysses.engine import split_align, split_placement
    rng = np.random.default_rng(3)
    for S in (32760, 75600, 118800, 8320, 1000):
        a = split_align(S)
        assert a == (256 if S >= 4096 else 32)
        for P in (2, 3, 4, 8):
            for _ in range(20):
                H = int(rng.choice([12, 24, 40]))
                e = [int(x) for x in rng.integers(0, 3, H)]
                order, counts, parts = split_placement(e, [5.6, 1.4, 1.0], P, S, 1, align=a)
                for h in set(order):
                    rs = sorted(parts[i] or (0, S) for i in range(len(order)) if order[i] == h)
                    assert rs[0][0] == 0 and rs[-1][1] == S and all(x[1] == y[0] for x, y in zip(rs, rs[1:]))
                    assert all(t0 % a == 0 and (t1 == S or t1 % a == 0) and t1 - t0 >= a for t0, t1 in rs), (S, P, rs)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_exchange_selfcheck_passes_and_catches_a_misordered_placement(world):
    ret = mp.Manager().dict()
    mp.spawn(_selfcheck_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    for r in range(world):
        for key, (ok, nb, ms) in ret[r].items():
            assert nb and ms, (r, key)
            assert ok == (not key[2]), (r, key, ok)  # break_order -> the check fails on EVERY rank (MIN all-reduce)


@pytest.mark.parametrize("world", [2, 4])
def test_uneven_head_placement_round_trip(world):
    ret = mp.Manager().dict()
    mp.spawn(_uneven_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert all(ret[r] for r in range(world)), dict(ret)


def test_balanced_placement_beats_equal_head_counts_on_skewed_mixes():
    from vorta_amd.ulysses import balanced_head_order, balanced_placement
    cost = [7.26, 1.82, 1.33]  # Hunyuan-129f: full / coreset / sliding-tile TFLOP per head
    rng = np.random.default_rng(5)
    for n0, n1, n2, P in ((4, 8, 12, 8), (8, 8, 8, 8), (3, 6, 15, 4), (14, 13, 13, 8)):
        e = rng.permutation([0] * n0 + [1] * n1 + [2] * n2)
        H = len(e)
        order, counts = balanced_placement(e, cost, P)
        assert sorted(order) == list(range(H)) and sum(counts) == H and min(counts) >= 1
        st = np.cumsum([0] + counts)
        uneven = max(sum(cost[e[h]] for h in order[st[j]:st[j + 1]]) for j in range(P))
        o2 = balanced_head_order(e, cost, P)
        even = max(sum(cost[e[h]] for h in o2[j * (H // P):(j + 1) * (H // P)]) for j in range(P))
        assert uneven <= even + 1e-9
        if (n0, n1, n2) == (4, 8, 12):  # 24 heads on 8 ranks, 4 full-attention heads: 1.33 of the mean with 3 heads each
            mean = sum(cost[x] for x in e) / P
            assert even / mean > 1.3 and uneven / mean < 1.05
    order, counts = balanced_placement([0] * 8, cost, 8, groups=3)  # groups clamp to the smallest head count
    assert counts == [1] * 8


def test_balanced_head_order_with_slot_groups():
    from vorta_amd.ulysses import balanced_head_order, slot_groups
    rng = np.random.default_rng(3)
    cost = [7.26, 1.82, 1.33]
    for P, G in ((2, 2), (2, 3), (4, 2), (4, 3), (8, 2), (2, 5), (4, 4)):
        e = rng.permutation([0] * 8 + [1] * 8 + [2] * 8)
        plain, grouped = balanced_head_order(e, cost, P), balanced_head_order(e, cost, P, groups=G)
        Hl = 24 // P
        sg = slot_groups(Hl, G)  # as equal as Hl allows, larger groups first (Hl = 3, G = 2: 2 + 1)
        assert sg[0][0] == 0 and sg[-1][1] == Hl and all(a[1] == b[0] for a, b in zip(sg, sg[1:]))
        assert max(b - a for a, b in sg) - min(b - a for a, b in sg) <= 1
        for j in range(P):  # same heads per rank as without groups; groups of a rank carry near-equal cost per slot
            assert sorted(grouped[j * Hl:(j + 1) * Hl]) == plain[j * Hl:(j + 1) * Hl]
            loads = [sum(cost[e[h]] for h in grouped[j * Hl + a:j * Hl + b]) / (b - a) for a, b in sg]
            assert max(loads) - min(loads) <= max(cost)
            for a, b in sg:
                assert grouped[j * Hl + a:j * Hl + b] == sorted(grouped[j * Hl + a:j * Hl + b])
    assert slot_groups(5, 2) == [(0, 3), (3, 5)] and slot_groups(3, 8) == [(0, 1), (1, 2), (2, 3)]


def test_balanced_head_order():
    from vorta_amd.ulysses import balanced_head_order
    cost = [7.26, 1.82, 1.33]
    rng = np.random.default_rng(0)
    for P in (2, 4, 8):
        e = rng.permutation(np.array([0] * 8 + [1] * 8 + [2] * 8))
        order = balanced_head_order(e, cost, P)
        assert sorted(order) == list(range(24))
        loads = [sum(cost[e[h]] for h in order[j * (24 // P):(j + 1) * (24 // P)]) for j in range(P)]
        assert max(loads) - min(loads) < 1e-9  # 8/8/8 splits evenly for P | 8
    with pytest.raises(AssertionError):
        balanced_head_order([0] * 12, cost, 8)


# ------------------------------------------------------------------ token-level shard of the pipeline call
class _PerTokenProcessor:
    """stands in for the attention processors on the CPU: per-token arithmetic + this rank's rows of the GLOBAL rotary
    table (narrowed exactly as the real processors narrow it, hunyuan.py:89-95) -- so a wrong shard, a local rotary
    table or a missing gather all change the result"""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, image_rotary_emb=None):
        from vorta_amd.ulysses import SP_STATE, shrink_dim
        cos = shrink_dim(image_rotary_emb[0], dim=0) if SP_STATE.enabled else image_rotary_emb[0]
        assert cos.shape[0] == hidden_states.shape[1]
        assert attention_mask.shape[-1] == cos.shape[0] * (SP_STATE.sp_size if SP_STATE.enabled else 1) + encoder_hidden_states.shape[1]
        pos = cos.float().mean(-1)[None, :, None].to(hidden_states.dtype)
        return torch.tanh(hidden_states) + pos, torch.tanh(encoder_hidden_states)


def _token_shard_worker(rank, world, port, ret):
    _init(rank, world, port)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _mini_diffusers as M
    from vorta_amd.patch import _engine as E
    from vorta_amd.patch import _pipeline as P
    from vorta_amd.patch.pipeline_hunyuan import sp_pipeline_call
    from vorta_amd.ulysses import SP_STATE

    class Pipe(M.MiniHunyuanPipeline):
        pass

    P.register_pipeline_class(Pipe)
    Pipe.__call__ = sp_pipeline_call
    torch.manual_seed(0)
    model = M.MiniHunyuanTransformer()
    E.context_of(model)
    E.clear_hooks(model)
    for block in list(model.transformer_blocks) + list(model.single_transformer_blocks):
        E.set_processor(block.attn, _PerTokenProcessor())
    E.install_sp_rope(model.rope, model)
    E.install_token_shard(model, model.transformer_blocks[0], model.norm_out)
    pipe = Pipe(model, "cpu")
    frames, h, w = 33, 2, 4  # 33 latent frames (129-frame video): no rank count but 1, 3, 11, 33 divides them
    g = torch.Generator().manual_seed(1)
    T = 6
    mask = torch.zeros((1, T))
    mask[:, :4] = 1
    args = dict(prompt_embeds=torch.randn((1, T, 24), generator=g), pooled_prompt_embeds=torch.randn((1, 16), generator=g),
                prompt_attention_mask=mask, height=h, width=w, num_frames=frames, num_inference_steps=2,
                output_type="latent", return_dict=False)
    full = pipe(**args, generator=torch.Generator().manual_seed(7))[0]
    SP_STATE.setup_sp_group(world)
    part = pipe(**args, generator=torch.Generator().manual_seed(7))[0]
    err = float((part - full).abs().max())
    # without a generator the ranks agree on a seed (pipeline_hunyuan.py:76-83)
    a = pipe(**args)[0]
    gathered = [torch.empty_like(a) for _ in range(world)]
    dist.all_gather(gathered, a)
    refused = False
    try:  # 33 * 2 * 4 = 264 tokens: 16 ranks would not divide them -- here: make the count odd
        pipe(**dict(args, height=1, width=1, num_frames=world + 1), generator=torch.Generator().manual_seed(7))
    except ValueError:
        refused = True
    incoherent = False
    try:  # a generator seeded per rank: every rank would denoise another video outside its own chunk -- refused at the first cut
        pipe(**args, generator=torch.Generator().manual_seed(100 + rank))
    except RuntimeError as e:
        incoherent = "different latents" in str(e)
    again = pipe(**args, generator=torch.Generator().manual_seed(7))[0]  # and the model is usable afterwards
    refused = refused and incoherent and torch.equal(again, part)
    ret[rank] = (err, float(full.abs().max()), tuple(part.shape), all(torch.equal(gathered[0], x) for x in gathered), refused)
    dist.barrier()
    SP_STATE.cleanup()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_pipeline_token_shard_33_frames(world):
    """the pipeline call under sequence parallelism with a frame count no rank count divides: every rank keeps the whole
    latent, the transformer cuts and re-joins its token sequence (vorta_amd/patch/_engine.py: install_token_shard)"""
    ret = mp.Manager().dict()
    mp.spawn(_token_shard_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    for r in range(world):
        err, mag, shape, same_seed, refused = ret[r]
        assert err <= 1e-5 * max(mag, 1.0), (r, err)
        assert shape == (1, 4, 33, 2, 4) and same_seed and refused


def _coherence_worker(rank, world, port, ret):
    _init(rank, world, port)
    from vorta_amd.patch._engine import check_rank_coherence
    from vorta_amd.ulysses import SP_STATE
    SP_STATE.setup_sp_group(world)
    N = 12_000_000  # the size class where a checksum goes blind: sqrt(N) / N = 3e-4
    res = {}
    same = torch.randn(N, generator=torch.Generator().manual_seed(5)).view(1, -1, 3000)
    # identical latents whose embedding went through another kernel on this rank: an ulp of bf16 apart, element by element
    jitter = (same.to(torch.bfloat16).float() * (1.0 + (0.004 if rank else 0.0))).view_as(same)
    other = torch.randn(N, generator=torch.Generator().manual_seed(100 + rank)).view(1, -1, 3000)
    for name, x in (("same", same), ("ulp apart", jitter), ("different seeds", other)):
        try:
            check_rank_coherence(x)
            res[name] = "ok"
        except RuntimeError as e:
            res[name] = "different latents" if "different latents" in str(e) else str(e)
    bad = same.clone()
    if rank == world - 1:
        bad[0, 17, 5] = float("nan")
    try:
        check_rank_coherence(bad)
        res["nan"] = "ok"
    except RuntimeError as e:
        res["nan"] = "not finite" if "not finite" in str(e) else str(e)
    # above 2^25 elements (the Wan-1.3B-81f hidden state, in bf16): a float32 sample index rounds to one past the end
    big = 50_319_360
    for name, seed in (("big same", 7), ("big different seeds", 200 + rank)):
        x = torch.randn(big, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).view(1, -1, 1536)
        try:
            check_rank_coherence(x)
            res[name] = "ok"
        except RuntimeError as e:
            res[name] = "different latents" if "different latents" in str(e) else str(e)
        except IndexError as e:
            res[name] = f"IndexError: {e}"
        del x
    # what the old checksum (signed sum and abs-sum to 1e-3 of the abs-sum) said about the per-rank seeds: nothing
    sums = torch.stack([other.sum(), other.abs().sum()]).reshape(1, 2)
    every = [torch.empty_like(sums) for _ in range(world)]
    dist.all_gather(every, sums)
    every = torch.cat(every)
    res["old checksum blind"] = bool(((every - every[:1]).abs() <= 1e-3 * every[:, 1].abs().max()).all())
    ret[rank] = res
    dist.barrier()
    SP_STATE.cleanup()


def test_rank_coherence_check_sees_per_rank_seeds_at_production_sizes():
    """at 1e7+ elements two differently seeded noise tensors agree in sum and abs-sum to 3e-4 -- under
    the old 1e-3 tolerance -- so per-rank seeds passed silently and every rank denoised another video.  The strided
    element sample refuses them at any size, lets identical latents an ulp apart through, and tells NaN apart."""
    ret = mp.Manager().dict()
    mp.spawn(_coherence_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    for r in range(2):
        assert ret[r] == {"same": "ok", "ulp apart": "ok", "different seeds": "different latents", "nan": "not finite",
                          "big same": "ok", "big different seeds": "different latents", "old checksum blind": True}, ret[r]


@pytest.mark.parametrize("n", [2 ** 24 + 1, 2 ** 25 + 1, 50_319_360, 91_238_400, 1, 2, 63, 64, 65, 1000])
def test_coherence_sample_indices_stay_inside_the_tensor(n):
    """the sample of check_rank_coherence: every index below n, the first 0, the last n - 1, strictly increasing, at every size
    (a float32 linspace put the last index AT n for n = 50_319_360: a device-side assert on the GPU)"""
    from vorta_amd.patch._engine import COHERENCE_SAMPLE, coherence_sample_indices
    idx = coherence_sample_indices(n)
    assert idx.dtype == torch.int64 and idx.numel() == min(COHERENCE_SAMPLE, n)
    assert int(idx[0]) == 0 and int(idx[-1]) == n - 1 and int(idx.max()) < n
    assert bool((idx[1:] > idx[:-1]).all())
