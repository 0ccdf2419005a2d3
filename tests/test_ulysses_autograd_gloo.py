"""world_size > 1 on CPU (gloo): the differentiable Ulysses exchange (vorta_amd/ulysses/autograd.py) and the autograd of
`comm.all_to_all_4D` / `comm.all_gather`, against the reference's rules (vorta/ulysses/utils.py:96-162).  No GPU, no HIP.

H = 6 heads, S/P = 8, T = 3, D = 8 on 2, 3 and 4 ranks -- 4 ranks hold 2, 2, 1, 1 heads (uneven counts).  float64, every
comparison exact: the exchange only moves rows, and the weights are small integers."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

H, SL, T, D = 6, 8, 3, 8


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _case(world):
    """global tensors every rank builds alike: x (H, S + T, D) (text rows last), cotangent G, per-head weights"""
    g = torch.Generator().manual_seed(11)
    S = SL * world
    x = torch.randint(-8, 9, (H, S + T, D), generator=g).double()
    G = torch.randint(-8, 9, (H, S + T, D), generator=g).double()
    w = torch.arange(2, 2 + H).double()
    return x, G, w


def _local(full, rank, world):
    S = SL * world
    return torch.cat([full[:, rank * SL:(rank + 1) * SL], full[:, S:]], dim=1).contiguous()


def _exchange_worker(rank, world, port, ret):
    _init(rank, world, port)
    from vorta_amd.ulysses import UlyssesLayout, gather_heads_autograd, scatter_heads_autograd
    P, S = world, SL * world
    counts = [H // P + (1 if j < H % P else 0) for j in range(P)]
    res = {"counts": counts}
    for name, order in (("natural", list(range(H))), ("permuted", [(5 * h + 2) % H for h in range(H)])):
        lay = UlyssesLayout(H, S, T, D, P, rank, "cpu", torch.float64, counts=counts)
        mine = order[lay.starts[rank]:lay.starts[rank + 1]]
        x, G, w = _case(world)
        xl = _local(x, rank, world).requires_grad_(True)
        Gl = _local(G, rank, world)
        # identity in place of attention: the round trip returns the shard and every head's text rows
        (buf,) = scatter_heads_autograd(lay, [xl], order)
        rm = lay.row_map.long()
        hv = lay.head_view(buf)
        landed = all(torch.equal(hv[i][rm], x[h]) for i, h in enumerate(mine))
        shard, text = gather_heads_autograd(lay, buf, order)
        ident = torch.equal(shard, xl[:, :SL].detach()) and torch.equal(text, xl[:, SL:].detach())
        # loss = <gather(w_h . scatter(x)), G>: row r of the buffer belongs to local head slot (r // Sl) % Hl
        (buf,) = scatter_heads_autograd(lay, [xl], order)
        slot = (torch.arange(lay.rows_total) // SL) % lay.Hl
        w_rows = w[torch.tensor(mine)][slot]
        out = gather_heads_autograd(lay, buf * w_rows[:, None], order, token_major=True)  # (Sl + T, H, D)
        (out * Gl.transpose(0, 1)).sum().backward()
        g = xl.grad
        want = w.view(H, 1, 1) * Gl
        own = torch.zeros(H, dtype=torch.bool)
        own[mine] = True
        res[name] = dict(landed=landed, ident=ident,
                         video=torch.equal(g[:, :SL], want[:, :SL]),
                         text_own=torch.equal(g[own][:, SL:], want[own][:, SL:]),
                         text_zero_elsewhere=bool((g[~own][:, SL:] == 0).all()),
                         n_own=int(own.sum()), text_grad=g[:, SL:].clone())
        # three tensors together: one backward exchange carries all of them
        xs = [(_local(x, rank, world) + t).requires_grad_(True) for t in range(3)]
        calls = []
        real = dist.all_to_all_single
        dist.all_to_all_single = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        try:
            bufs = scatter_heads_autograd(lay, xs, order)
            n_fwd = len(calls)
            sum(((t + 1) * b).sum() for t, b in enumerate(bufs)).backward()
        finally:
            dist.all_to_all_single = real
        res[name].update(three=all(torch.equal(xs[t].grad[:, :SL], torch.full((H, SL, D), t + 1.0).double()) for t in range(3)),
                         a2a_forward=n_fwd, a2a_backward=len(calls) - n_fwd)
    ret[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_differentiable_exchange(world):
    ret = mp.Manager().dict()
    mp.spawn(_exchange_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    x, G, w = _case(world)
    S = SL * world
    single = (w.view(H, 1, 1) * G)[:, S:]  # the single-process gradient of the text rows
    for name in ("natural", "permuted"):
        total = torch.zeros_like(single)
        for r in range(world):
            res = ret[r][name]
            assert res["landed"] and res["ident"], (world, r, name)                  # gather(scatter(x)) == x
            assert res["video"], (world, r, name)                                    # d video rows = w_h G on the shard
            assert res["text_own"] and res["text_zero_elsewhere"], (world, r, name)  # own heads' text rows, zeros elsewhere
            assert res["n_own"] == ret[r]["counts"][r]
            assert res["three"] and res["a2a_forward"] == 3 and res["a2a_backward"] == 3, (world, r, name, res)
            total += res["text_grad"]
        assert torch.equal(total, single), (world, name)                             # summed over ranks = one process
    assert ret[0]["counts"] == ([2, 2, 1, 1] if world == 4 else [H // world] * world)


def _comm_worker(rank, world, port, ret):
    _init(rank, world, port)
    from vorta_amd.ulysses import SP_STATE, all_gather, all_to_all_4D
    SP_STATE.setup_sp_group(world)
    P = world
    Hc = 2 * P  # the reference's collectives need P | H
    g = torch.Generator().manual_seed(5 + rank)
    ok = {}
    # seq -> head, then head -> seq: the gradient of either is the other applied to the cotangent (utils.py:111-120)
    x = torch.randint(-8, 9, (1, Hc, SL, D), generator=g).double().requires_grad_(True)
    y = all_to_all_4D(x, 1, 2)
    cy = torch.randint(-8, 9, tuple(y.shape), generator=g).double()
    (gx,) = torch.autograd.grad((y * cy).sum(), x)
    with torch.no_grad():
        ok["seq_to_head"] = torch.equal(gx, all_to_all_4D(cy, 2, 1))
    yl = y.detach().clone().requires_grad_(True)
    z = all_to_all_4D(yl, 2, 1)
    cz = torch.randint(-8, 9, tuple(z.shape), generator=g).double()
    (gy,) = torch.autograd.grad((z * cz).sum(), yl)
    with torch.no_grad():
        ok["head_to_seq"] = torch.equal(gy, all_to_all_4D(cz, 1, 2))
    ok["round_trip"] = torch.equal(z.detach(), x.detach())
    # <A x, c> = <x, A^T c> summed over the ranks: the adjoint identity of the pair of collectives
    lhs = torch.stack([(y.detach() * cy).sum(), (x.detach() * gx).sum()])
    dist.all_reduce(lhs)
    ok["adjoint"] = bool(lhs[0] == lhs[1])
    # all-gather: the gradient is this rank's slice of the cotangent, not a sum (utils.py:148-158)
    t = torch.randint(-8, 9, (1, 2, T, D), generator=g).double().requires_grad_(True)
    ta = all_gather(t, dim=1)
    ct = torch.randint(-8, 9, tuple(ta.shape), generator=torch.Generator().manual_seed(99)).double()  # replicated cotangent
    (gt,) = torch.autograd.grad((ta * ct).sum(), t)
    ok["all_gather"] = tuple(ta.shape) == (1, 2 * P, T, D) and torch.equal(gt, ct[:, 2 * rank:2 * rank + 2])
    ok["all_gather_forward"] = torch.equal(ta[:, 2 * rank:2 * rank + 2].detach(), t.detach())
    ret[rank] = ok
    dist.barrier()
    SP_STATE.cleanup()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_reference_collectives_carry_the_reference_autograd(world):
    ret = mp.Manager().dict()
    mp.spawn(_comm_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    for r in range(world):
        assert all(ret[r].values()), (world, r, dict(ret[r]))
