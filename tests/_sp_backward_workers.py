"""Workers of tests/test_hip_sp_soft_mixture_backward.py: what the gloo ranks that share the one GPU run (spawned processes
import this module), and the host-side check of the receive layout that tests/test_host_sp_backward.py runs without a GPU.

Cases, geometry and float64 references: tests/_sp_soft_mixture.py; rank set-up, gathering and assembly: the helpers of
tests/test_hip_sp_soft_mixture.py (imported, not restated)."""
import os

import torch

import _sp_soft_mixture as C

BWD_OPS = ("attn_bwd", "attn_bwd_stats", "attn_bwd_key_major", "attn_bwd_dq", "attn_bwd_dkv")
# what one recorded launch costs under each algorithm, in calls of vorta_amd.ops
EXPECTED = {"query_major": {"attn_bwd": 1},
            "key_major": {"attn_bwd_stats": 1, "attn_bwd_key_major": 1},
            "deterministic": {"attn_bwd_stats": 1, "attn_bwd_dq": 1, "attn_bwd_dkv": 1}}


def expected_calls(algorithm: str, n_launches: int) -> dict:
    return {n: EXPECTED[algorithm].get(n, 0) * n_launches for n in BWD_OPS}


class SpyBackwardOps:
    """counts the calls of the five backward entry points of vorta_amd.ops (routed._attn_bwd_by reads them off the module)
    and keeps the geometry of the float32 accumulators the deterministic passes were handed"""

    def __enter__(self):
        from vorta_amd import ops
        self.ops, self.stock = ops, {n: getattr(ops, n) for n in BWD_OPS}
        self.calls = {n: 0 for n in BWD_OPS}
        self.acc = {}

        def wrap(name, stock):
            def spy(*a, **kw):
                self.calls[name] += 1
                if name == "attn_bwd_dq":
                    self.acc["dq"] = (tuple(a[5].shape), tuple(a[5].stride()))
                elif name == "attn_bwd_dkv":
                    self.acc["dk"] = (tuple(a[5].shape), tuple(a[5].stride()))
                    self.acc["dv"] = (tuple(a[6].shape), tuple(a[6].stride()))
                return stock(*a, **kw)
            return spy

        for n in BWD_OPS:
            setattr(ops, n, wrap(n, self.stock[n]))
        return self

    def __exit__(self, *exc):
        for n in BWD_OPS:
            setattr(self.ops, n, self.stock[n])


# ------------------------------------------------------------------------------------------- the layout's precondition
def _one_to_one(heads, rows, shape, stride):
    """(head * stride_h + row * stride_s is one-to-one over heads x rows, every such row lies inside the view):
    heads (n,), rows (n, m) int64; shape / stride of the (heads, rows, D) float32 view, in elements"""
    addr = heads[:, None] * stride[0] + rows * stride[1]
    inside = bool((rows >= 0).all()) and bool((rows < shape[1]).all()) and bool((heads < shape[0]).all())
    return torch.unique(addr).numel() == addr.numel(), inside


def key_lists_of(c, n_heads: int):
    """the key lists of one recorded launch as (n_heads, n_kv) row tables, one per dK / dV kernel launch"""
    n_kv, kv = c["n_kv"], c["kv_rows"].cpu().long()
    sg = c.get("kv_rows_stride_g", 0) or 0
    if sg > 0:  # one list per query group, shared by the head slots
        if c.get("q_block_table") is not None:
            n_lists = c["n_key_lists"]
        else:
            n_lists = -(-c["n_q"] // (c.get("q_group_len") or c["n_q"]))
        flat = kv.reshape(-1)
        return [flat[g * sg: g * sg + n_kv][None].expand(n_heads, n_kv) for g in range(n_lists)]
    if kv.dim() == 1:  # shared by the head slots
        return [kv[:n_kv][None].expand(n_heads, n_kv)]
    return [kv[:n_heads, :n_kv]]


def layout_precondition(launches, acc):
    """What `deterministic` needs of the launches one rank recorded, computed on the host from the row tables (already
    composed with the row map), the head lists and the accumulators' head views (`acc`: name -> (shape, stride)):
      (a) the first n_kv rows of every key list are distinct, a head list names distinct heads;
      (b) head * stride_h + row * stride_s is one-to-one over the (slot, query row) pairs a launch names for dq, and over
          the (slot, key row) pairs of ONE key list for dk and dv -- the head views of a receive buffer overlap."""
    res = dict(launches=len(launches), key_lists=0, rows_distinct=True, heads_distinct=True, dq_one_to_one=True,
               dkv_one_to_one=True, inside=True, text_rows_seen=False)
    for c in launches:
        n_heads = c.get("n_heads")
        if n_heads is None:
            n_heads = c["head_list"].numel() if c.get("head_list") is not None else c["q"].shape[0]
        heads = c["head_list"].cpu().long()[:n_heads] if c.get("head_list") is not None else torch.arange(n_heads)
        res["heads_distinct"] &= torch.unique(heads).numel() == n_heads
        # dq: the positions that take a gradient (below q_valid), through the slot's query rows
        n_named = min(c["n_q"], c["n_q"] if c.get("q_valid") is None else c["q_valid"])
        qr = c["q_rows"].cpu().long()
        qr = qr[:n_named][None].expand(n_heads, n_named) if qr.dim() == 1 else qr[:n_heads, :n_named]
        ok, inside = _one_to_one(heads, qr, *acc["dq"])
        res["dq_one_to_one"] &= ok
        res["inside"] &= inside
        for rows in key_lists_of(c, n_heads):
            res["key_lists"] += 1
            res["rows_distinct"] &= all(torch.unique(r).numel() == r.numel() for r in rows)
            for name in ("dk", "dv"):
                ok, inside = _one_to_one(heads, rows, *acc[name])
                res["dkv_one_to_one"] &= ok
                res["inside"] &= inside
        if c.get("tag") == "full" and c["n_q"] > C.S:
            res["text_rows_seen"] = True
    return {k: (bool(v) if isinstance(v, (bool, torch.Tensor)) else v) for k, v in res.items()}


# ------------------------------------------------------------------------------------------------------------- workers
def _clear_selection():
    from vorta_amd import routed
    routed._attention_backward = None
    os.environ.pop("VORTA_ATTENTION_BACKWARD", None)


def _run_operator(model, tensors, rank, P, backward=None, repeats=1, between=None):
    """forward + `repeats` backward passes of ONE forward on this rank's shard (every pass zeroes accumulators of its own);
    `between()` runs after the forward and before the first backward.  Returns the pieces `_assemble` reads (the first
    pass's gradients), every pass's gradients, the ops calls of the backward passes and the recorded launches."""
    from vorta_amd.routed import sp_soft_mixture_attention_autograd
    q, k, v, sc, cot = tensors
    T, te = C.text_of(model)
    kw = dict(C.geometry_kw(), model=model, text_valid=te)
    if backward is not None:
        kw["backward"] = backward
    loc = [C.shard(x, rank, P).requires_grad_(True) for x in (q, k, v)]
    s = sc.clone().requires_grad_(True)
    with C.RecordSp() as rec:
        out = sp_soft_mixture_attention_autograd(*loc, T, s, **kw)
    assert len(rec.calls) == 1
    if between is not None:
        between()
    loss = (out * C.shard(cot, rank, P, dim=1)).sum()
    passes = []
    with SpyBackwardOps() as spy:
        for i in range(repeats):
            passes.append(torch.autograd.grad(loss, loc + [s], retain_graph=i + 1 < repeats))
    torch.cuda.synchronize()
    return dict(out=out.detach(), grads=list(passes[0][:3]), dsc=passes[0][3], call=rec.calls[0], passes=passes,
                calls=dict(spy.calls), acc=dict(spy.acc), n_launches=len(rec.calls[0][0]))


def gradient_worker(rank, world, port, ret, model, H, dtype_name, algorithm, repeats):
    """one case of the operator under `algorithm`: the forward under all three algorithms, `repeats` backward passes, the
    layout's precondition on this rank's launches; rank 0 assembles and compares against float64"""
    import test_hip_sp_soft_mixture as M
    dist, SP = M._setup(rank, world, port)
    _clear_selection()
    from vorta_amd.attention._sp import _mixture_placement
    from vorta_amd.routed import ATTENTION_BACKWARDS, sp_soft_mixture_attention_autograd
    dtype = M.DTYPES[dtype_name]
    T, te = C.text_of(model)
    tensors = C.operator_case(model, H, dtype)
    q, k, v, sc, cot = tensors
    piece = _run_operator(model, tensors, rank, world, backward=algorithm, repeats=repeats)
    # the forward does not depend on the backward's algorithm
    with torch.no_grad():
        others = [sp_soft_mixture_attention_autograd(*[C.shard(x, rank, world) for x in (q, k, v)], T, sc, **C.geometry_kw(),
                                                    model=model, text_valid=te, backward=a)
                  for a in ATTENTION_BACKWARDS if a != algorithm]
    piece["same_as_no_grad"] = all(torch.equal(piece["out"], o) for o in others)
    same_passes = {n: all(torch.equal(p[i], piece["passes"][0][i]) for p in piece["passes"])
                   for i, n in enumerate(("dq", "dk", "dv", "dscores"))}
    pre = layout_precondition(piece["call"][0], piece["acc"]) if algorithm == "deterministic" else None
    counts = _mixture_placement(H, world)[1]
    head0 = (sum(counts[:rank]), sum(counts[:rank + 1]))
    mine = M._gather(dist, dict(same_passes=same_passes, pre=pre, calls=piece["calls"], n_launches=piece["n_launches"]))
    glob = M._assemble(dist, piece, H, world, T, head0)
    if rank == 0:
        res = dict(counts=counts, zeros_ok=glob["zeros_ok"], forward_same=glob["same_as_no_grad"], per_rank=mine, repeats=repeats)
        g64, o64 = C.reference_grads(q, k, v, sc, cot, glob["launches"], torch.float64)
        g16, _ = C.reference_grads(q, k, v, sc, cot, glob["launches"], dtype)
        res["restated_forward"] = C.rel_err(glob["out"], o64)
        bwd = {}
        for name, got, r64, r16 in zip(("dq", "dk", "dv"), glob["grads"], g64, g16):
            bwd[name + " video"] = (C.rel_err(got[:, :C.S], r64[:, :C.S]), C.rel_err(r16[:, :C.S], r64[:, :C.S]))
            if T:
                bwd[name + " text"] = (C.rel_err(got[:, C.S:], r64[:, C.S:]), C.rel_err(r16[:, C.S:], r64[:, C.S:]))
        bwd["dscores"] = (C.rel_err(glob["dsc"], g64[3]), C.rel_err(g16[3], g64[3]))
        res["bwd"] = bwd
        # beside it (a figure, not a claim): the single-process operator under the same algorithm, bit for bit.  Only one
        # rank holds a non-zero text row of a head, so the sum over the ranks in `_assemble` is exact.
        from vorta_amd.routed import geometry_for, soft_mixture_attention_autograd
        L = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
        geom = geometry_for(C.LATENT, C.TILE, C.WINDOW, C.GROUP, C.RATE, C.dev())
        one = soft_mixture_attention_autograd(*L, geom, model=model, text_len=T, text_valid=te, backward=algorithm)
        (one * cot.transpose(1, 2)).sum().backward()
        torch.cuda.synchronize()
        res["bits_equal_single_process"] = {n: torch.equal(g.to(dtype), x.grad[0])
                                            for n, g, x in zip(("dq", "dk", "dv"), glob["grads"], L)}
        ret["res"] = res
    dist.barrier()
    SP.cleanup()


def dispatch_worker(rank, world, port, ret, model):
    """the three selection routes, and that the choice is read when the forward runs; bf16, H = 4"""
    import test_hip_sp_soft_mixture as M
    dist, SP = M._setup(rank, world, port)
    from vorta_amd import routed
    tensors = C.operator_case(model, 4, torch.bfloat16)
    out = {}

    def scenario(name, keyword=None, switch=None, env=None, after=None):
        _clear_selection()
        if switch is not None:
            routed.set_attention_backward(switch)
        if env is not None:
            os.environ["VORTA_ATTENTION_BACKWARD"] = env
        piece = _run_operator(model, tensors, rank, world, backward=keyword,
                              between=None if after is None else (lambda: routed.set_attention_backward(after)))
        out[name] = dict(calls=piece["calls"], n_launches=piece["n_launches"])
        return piece

    scenario("nothing set")
    by_keyword = scenario("keyword deterministic", keyword="deterministic")
    scenario("keyword key_major", keyword="key_major")
    by_switch = scenario("switch deterministic", switch="deterministic")
    scenario("switch key_major", switch="key_major")
    scenario("environment deterministic", env="deterministic")
    scenario("environment key_major", env="key_major")
    scenario("keyword deterministic over switch key_major", keyword="deterministic", switch="key_major")
    scenario("switch over environment", switch="query_major", env="deterministic")
    scenario("forward deterministic, then switched to query_major", switch="deterministic", after="query_major")
    scenario("forward with nothing set, then switched to deterministic", after="deterministic")
    _clear_selection()
    # one algorithm, two routes to it: the same kernels on the same buffers, hence the same bits
    same = all(torch.equal(a, b) for a, b in zip(by_keyword["passes"][0], by_switch["passes"][0]))
    ret[rank] = dict(scenarios=out, keyword_equals_switch=same)
    dist.barrier()
    SP.cleanup()


def processor_worker(rank, world, port, ret):
    """`differentiable=True` Train processors (Wan, Hunyuan single block) on this rank's shard under the process-wide switch"""
    import test_hip_processors_grad as G
    import test_hip_sp_soft_mixture as M
    G.T, G.TE = C.T_HY, C.TE_HY  # (this process only: a spawned worker)
    dist, SP = M._setup(rank, world, port)
    from vorta_amd import routed
    dtype = torch.bfloat16
    Sl = G.S // world
    out = {}
    for which in ("wan", "hunyuan_single"):
        if which == "wan":
            from vorta_amd.attention import WanAttnProcessorTripleTrain as Train
            attn = G._WanAttn(dtype, seed=41)
            hidden, _, freqs, _, score, kw = G._wan_case(dtype, 9)
            call = lambda p, h, sc: p(attn, h, None, None, freqs, routing_score=sc, **kw)  # noqa: E731
        else:
            from vorta_amd.attention import HunyuanVideoFlashAttnProcessorTripleTrain as Train
            attn = G._HyAttn(False, dtype, seed=31)
            hidden, enc, rope, mask, score, kw = G._hy_case(dtype, 7)
            call = lambda p, h, sc: p(attn, h, enc, mask, rope, routing_score=sc, **kw)  # noqa: E731
        proc = Train(differentiable=True)
        for switch in (None, "deterministic", "key_major"):
            _clear_selection()
            if switch is not None:
                routed.set_attention_backward(switch)
            h_loc = hidden[:, rank * Sl:(rank + 1) * Sl].clone().requires_grad_(True)
            s = score.clone().requires_grad_(True)
            with C.RecordSp() as rec:
                outs = call(proc, h_loc, s)
            outs = outs if isinstance(outs, tuple) else (outs,)
            with SpyBackwardOps() as spy:
                sum(o.float().sum() for o in outs).backward()
            torch.cuda.synchronize()
            assert len(rec.calls) == 1
            out[f"{which} {switch or 'nothing set'}"] = dict(
                calls=dict(spy.calls), n_launches=len(rec.calls[0][0]),
                finite=bool(torch.isfinite(h_loc.grad).all()) and bool(torch.isfinite(s.grad).all()) and bool(h_loc.grad.any()))
    _clear_selection()
    ret[rank] = out
    dist.barrier()
    SP.cleanup()
