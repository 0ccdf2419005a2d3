"""CPU: the two host pieces of router training under sequence parallelism (vorta_amd/patch/_engine.py) --
`all_reduce_router_grads(model)` on a gloo world of two with hand-set gradients, and `token_sharded(model)` on the stubbed
mini models of tests/test_host_patch_training.py (its builders, imported: every attention processor is a torch stand-in, so
no kernel runs): what the context refuses and restores, that a forward reads the mode once, how often the ranks' tokens are
compared, and that a frame count the ranks do not divide is refused by name outside it."""
import os
import socket
import time

import pytest
import torch

import _mini_diffusers as M
import test_host_patch_training as HT


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(rank, world, port):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vorta_amd.ulysses import SP_STATE
    return dist, SP_STATE


def _run(target, world=2, limit=120):
    """tests/test_hip_sp_soft_mixture.py `_run` on the CPU: one time limit for the spawn, a failed or late worker fails"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=target, args=(r, world, port, ret)) for r in range(world)]
        for p in procs:
            p.start()
        deadline = time.monotonic() + limit
        for p in procs:
            p.join(timeout=max(0.0, deadline - time.monotonic()))
        late = [p for p in procs if p.is_alive()]
        for p in late:
            p.kill()
            p.join()
        assert not late and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        return dict(ret)


# --------------------------------------------------------------------------------------------------- all_reduce_router_grads
def _router_params(model):
    from vorta_amd.patch._engine import installed_routers
    return [p for r in installed_routers(model) for p in r.parameters()]


def _set_grads(model, rank):
    """gradient of parameter i on `rank`: (i + 1) * (rank + 1) + 0.25 * rank, every element -- exact in bf16"""
    for i, p in enumerate(_router_params(model)):
        p.grad = torch.full_like(p, (i + 1) * (rank + 1) + 0.25 * rank)


def _reduce_worker(rank, world, port, ret):
    from vorta.patch import all_reduce_router_grads
    dist, SP = _setup(rank, world, port)
    res = {}
    for family in ("hunyuan", "wan"):
        model = (HT._hy if family == "hunyuan" else HT._wan)()[0]
        params = _router_params(model)
        res[family + " count"] = len(params)
        other = model.proj_out.weight
        other.grad = torch.full_like(other, float(rank + 1))
        _set_grads(model, rank)
        all_reduce_router_grads(model)  # sequence parallelism is not enabled yet: nothing happens, nothing is required
        res[family + " noop"] = all(bool((p.grad == (i + 1) * (rank + 1) + 0.25 * rank).all()) for i, p in enumerate(params))
        params[0].grad = None
        all_reduce_router_grads(model)  # (not even a gradient)
        SP.setup_sp_group(world)
        try:
            _set_grads(model, rank)
            all_reduce_router_grads(model, op="sum")
            # ranks 0 and 1: (i + 1) * 1 + (i + 1) * 2 + 0.25
            res[family + " sum"] = all(bool((p.grad == 3 * (i + 1) + 0.25).all()) for i, p in enumerate(params))
            res[family + " dtype kept"] = all(p.grad.dtype == p.dtype and p.grad.shape == p.shape for p in params)
            _set_grads(model, rank)
            all_reduce_router_grads(model, op="avg")
            res[family + " avg"] = all(bool((p.grad == 1.5 * (i + 1) + 0.125).all()) for i, p in enumerate(params))
            res[family + " others untouched"] = bool((other.grad == rank + 1).all())
            params[3].grad = None  # on every rank: the refusal comes before the collective
            try:
                all_reduce_router_grads(model)
                res[family + " missing"] = "not refused"
            except RuntimeError as e:
                res[family + " missing"] = str(e)
            try:
                all_reduce_router_grads(model, op="max")
                res[family + " op"] = "not refused"
            except ValueError as e:
                res[family + " op"] = str(e)
        finally:
            SP._enabled = False  # the next family's no-op case; the group stays for the second round
    ret[rank] = res
    dist.barrier()
    SP._enabled = True
    SP.cleanup()


def test_all_reduce_router_grads_on_a_gloo_world_of_two():
    ret = _run(_reduce_worker)
    for rank in range(2):
        res = ret[rank]
        for family, layers in (("hunyuan", 4), ("wan", 3)):
            assert res[family + " count"] == 2 * layers  # weight and bias of every block's router
            for what in ("noop", "sum", "avg", "dtype kept", "others untouched"):
                assert res[f"{family} {what}"] is True, (rank, family, what)
            # the second parameter of the second router, by name
            assert "router of block 1: linear.bias" in res[family + " missing"], res[family + " missing"]
            assert "'sum' or 'avg'" in res[family + " op"]


def test_all_reduce_router_grads_refuses_an_unpatched_model():
    from vorta.patch import all_reduce_router_grads
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        all_reduce_router_grads(M.MiniWanTransformer())


# ------------------------------------------------------------------------------------------------------------ token_sharded
def test_token_sharded_refuses_an_unpatched_model_and_restores_the_flag_after_an_exception():
    from vorta.patch import token_sharded
    from vorta_amd.patch import _engine as E
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        with token_sharded(M.MiniHunyuanTransformer()):
            pass
    model, blocks, inp, kw, log, _ = HT._hy(seed=13)
    ctx = E.context_of(model)
    assert ctx.sp_token_shard is False
    with pytest.raises(KeyError):
        with token_sharded(model, check=False):
            assert ctx.sp_token_shard and ctx.sp_coherent
            with token_sharded(model):  # nests; asks for the comparison again
                assert ctx.sp_token_shard and not ctx.sp_coherent
            assert ctx.sp_token_shard and ctx.sp_coherent
            raise KeyError("inside")
    assert ctx.sp_token_shard is False and ctx.sp_coherent is False
    # without sequence parallelism the context changes no forward
    with token_sharded(model):
        out = model(**inp, return_dict=False, self_attention_kwargs=kw)
    assert out[0].shape == inp["hidden_states"].shape and len(log) == len(blocks)
    assert E.context_of(model).token_shard_of() is False


class _ShapeStub(HT._Stub):
    """tests/test_host_patch_training.py `_Stub` that also notes how many video tokens and which rotary table it was handed"""

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask, rotary, **kw):
        out = super().__call__(attn, hidden_states, encoder_hidden_states, attention_mask, rotary, **kw)
        self.log[-1].update(tokens=hidden_states.shape[1], rotary=rotary)
        return out


def _restub(blocks, log):
    import inspect
    for b in blocks:
        bound = b.attn.processor
        bound.inner = _ShapeStub(log, bound.layer)
        bound._accepted = set(inspect.signature(HT._Stub.__call__).parameters)


def _shard_worker(rank, world, port, ret):
    from vorta.patch import token_sharded
    from vorta.patch.utils import prepare_hunyuan_self_attn_kwargs
    from vorta_amd.patch import _engine as E
    dist, SP = _setup(rank, world, port)
    model, blocks, inp, kw, log, _ = HT._hy(seed=21)
    _restub(blocks, log)
    ctx = E.context_of(model)
    # (grad mode throughout: under no_grad the scores come from the route plan, a kernel)
    whole = model(**inp, return_dict=False, self_attention_kwargs=kw)[0].detach()
    del log[:]
    SP.setup_sp_group(world)
    res = {}
    compared = []
    stock = E.check_rank_coherence
    E.check_rank_coherence = lambda x: (compared.append(tuple(x.shape)), stock(x))[1]
    # 1. two forwards inside one context: whole latents in, S / P tokens in every block, whole outputs, ONE comparison
    with token_sharded(model):
        a = model(**inp, return_dict=False, self_attention_kwargs=kw)[0]
        b = model(**inp, return_dict=False, self_attention_kwargs=kw)[0]
        res["modes inside"] = ctx.sp_token_shard
    res["shapes"] = (tuple(a.shape), tuple(b.shape), tuple(whole.shape))
    res["tokens"] = sorted({c["tokens"] for c in log})
    res["calls"] = len(log)
    res["compared"] = list(compared)
    res["rotary rows"] = log[0]["rotary"][0].shape[0]
    # the stand-in attention is row-wise, so the token-sharded forward states the single-process one: 16-bit GEMMs over
    # another row count may round another way, a cut or a gather at the wrong place is wrong by the output's own size
    res["err"] = float((a.float() - whole.float()).norm() / whole.float().norm())
    # 2. the mode is the forward's: the flag drops after the first block and the gather still runs; a later look-up by the
    # rotary table of that forward (what a recomputed block is handed) still says token shard, outside the context
    del log[:]
    hook = blocks[0].register_forward_hook(lambda m, args, out: setattr(ctx, "sp_token_shard", False))
    with token_sharded(model, check=False):
        c = model(**inp, return_dict=False, self_attention_kwargs=kw)[0]
    hook.remove()
    res["flag dropped mid-forward"] = (tuple(c.shape), sorted({x["tokens"] for x in log}), bool(torch.equal(c, a)))
    res["compared after check=False"] = len(compared)
    res["flag after"] = (ctx.sp_token_shard, ctx.sp_coherent)
    res["mode on record"] = (ctx.current is None, ctx.token_shard_of((log[0]["rotary"],)), ctx.token_shard_of())
    # 3. a new entry compares again
    with token_sharded(model):
        model(**inp, return_dict=False, self_attention_kwargs=kw)
    res["compared after re-entry"] = len(compared)
    # 4. outside the context a forward is frame-sharded: this rank's frames in, the global rotary table, its frames out
    del log[:]
    f = inp["hidden_states"].shape[2] // world
    mine = dict(inp, hidden_states=inp["hidden_states"][:, :, rank * f:(rank + 1) * f].contiguous())
    d = model(**mine, return_dict=False, self_attention_kwargs=kw)[0]
    res["frame shard"] = (tuple(d.shape), sorted({x["tokens"] for x in log}), log[0]["rotary"][0].shape[0], len(compared))
    res["frame err"] = float((d.float() - whole[:, :, rank * f:(rank + 1) * f].float()).norm() / whole.float().norm())
    # 5. three latent frames on two ranks: refused by name outside the context, taken inside (144 tokens = 2 x 72)
    lat = (3, 6, 8)
    kw3 = prepare_hunyuan_self_attn_kwargs(dict(HT.KW, latent_shape=lat, tile_size=(1, 3, 4), lowres_window_size=(3, 3, 2)),
                                           torch.device("cpu"))
    odd = dict(inp, hidden_states=inp["hidden_states"][:, :, :3].contiguous())
    try:
        model(**dict(odd, hidden_states=odd["hidden_states"][:, :, :2]), return_dict=False, self_attention_kwargs=kw3)
        res["odd frames"] = "not refused"
    except ValueError as e:
        res["odd frames"] = str(e)
    del log[:]
    with token_sharded(model):
        e3 = model(**odd, return_dict=False, self_attention_kwargs=kw3)[0]
    res["odd frames inside"] = (tuple(e3.shape), sorted({x["tokens"] for x in log}))
    E.check_rank_coherence = stock
    ret[rank] = res
    dist.barrier()
    SP.cleanup()


def test_token_sharded_forwards_on_a_gloo_world_of_two():
    ret = _run(_shard_worker)
    whole = (1, 4, 4, 6, 8)
    for rank in range(2):
        res = ret[rank]
        assert res["modes inside"] is True
        assert res["shapes"] == (whole, whole, whole)
        assert res["tokens"] == [96] and res["calls"] == 8  # 4 blocks, two forwards, 192 / 2 tokens
        assert res["compared"] == [(1, 192, 512)], "one comparison of the ranks' tokens per entry, not per forward"
        assert res["rotary rows"] == 192  # the global table: the processors narrow it
        # bf16 has 8 bits: a row-wise forward over 96 rows instead of 192 differs by roundings, 2^-8 each, in a few of its
        # elements at most; a misplaced cut or gather is an error of order 1
        assert res["err"] <= 2.0 ** -6, res["err"]
        assert res["flag dropped mid-forward"] == (whole, [96], True)
        assert res["compared after check=False"] == 1
        assert res["flag after"] == (False, False)
        assert res["mode on record"] == (True, True, False)
        assert res["compared after re-entry"] == 2
        assert res["frame shard"] == ((1, 4, 2, 6, 8), [96], 192, 2)
        assert res["frame err"] <= 2.0 ** -6, res["frame err"]
        assert "frame" in res["odd frames"] and " 3 " in res["odd frames"], res["odd frames"]
        assert res["odd frames inside"] == ((1, 4, 3, 6, 8), [72])
