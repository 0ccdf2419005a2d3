"""GPU: the soft mixture (router training) under sequence parallelism -- `sp_soft_mixture_attention[_autograd]` and the
Train processors with `differentiable=True` -- on gloo ranks that share the one GPU (host-staged transport, the spawn
pattern of tests/test_hip_patch.py), plus one case on a real RCCL group of one rank.

Truth and bounds (none of them new):
  * forward: the float64 oracle (`oracle.soft_mixture_attention`); the sequence-parallel error may be at most 2 x the
    single-process error -- the factor this project uses between two 16-bit evaluations of one formula;
  * backward: float64 autograd of the restatement of the recorded launches (tests/_attn_restate.py; the coreset ranking and
    the sliding tables are constants of the backward); per gradient, error <= 2 x that of torch's own 16-bit autograd on the
    same restatement (tests/test_hip_attention_bwd.py "bound 2", tests/test_hip_processors_grad.py).
Shapes: tests/_sp_soft_mixture.py.  Rank 0 of every case gathers the ranks' pieces and computes the references; the parent
asserts on the figures.  VORTA_SP_SOFT_MIXTURE_ACCURACY_OUT names a file that receives them."""
import json
import os
import socket
import subprocess
import sys
import time

import pytest
import torch

import _sp_soft_mixture as C

pytestmark = pytest.mark.gpu
ROOT = C.ROOT
FIGURES = []  # (kind, case, name, e, e_yardstick) of every bound checked in this module
BITS = {}     # case -> forward bits equal to the single-process operator's
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ------------------------------------------------------------------------------------------------------------- workers
def _setup(rank, world, port):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from vorta_amd.ulysses import SP_STATE
    SP_STATE.setup_sp_group(world)
    return dist, SP_STATE


def _gather(dist, obj):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def _np(t):
    return t.detach().float().cpu().numpy()


def _sp_operator(model, q, k, v, sc, cot, rank, P, record=True):
    """forward (no_grad and grad form) + backward of the operator on this rank's shard; returns its pieces"""
    from vorta_amd.routed import sp_soft_mixture_attention, sp_soft_mixture_attention_autograd
    T, te = C.text_of(model)
    kw = dict(C.geometry_kw(), model=model, text_valid=te)
    loc = [C.shard(x, rank, P).requires_grad_(True) for x in (q, k, v)]
    s = sc.clone().requires_grad_(True)
    out0 = sp_soft_mixture_attention(*[x.detach() for x in loc], T, sc, **kw)
    with C.RecordSp() as rec:
        out = sp_soft_mixture_attention_autograd(*loc, T, s, **kw)
    (out * C.shard(cot, rank, P, dim=1)).sum().backward()
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    return dict(out=out.detach(), same_as_no_grad=torch.equal(out, out0), grads=[x.grad for x in loc], dsc=s.grad, call=rec.calls[0])


def _assemble(dist, piece, H, P, T, head0):
    """every rank's pieces -> the global tensors (on rank 0's device): out (H, S+T, D), dq/dk/dv (H, S+T, D) with the video
    shards concatenated and the text rows summed, dscores summed; + the zero checks of the rows a rank does not own"""
    Sl = C.S // P
    mine = torch.zeros(H, dtype=torch.bool)
    mine[head0[0]:head0[1]] = True
    zeros_ok = bool((piece["dsc"][0][~mine] == 0).all()) and bool((piece["dsc"][0][mine] != 0).any())
    if T:
        zeros_ok = zeros_ok and all(bool((g[0][~mine][:, Sl:] == 0).all()) for g in piece["grads"])
    got = _gather(dist, dict(out=_np(piece["out"][0]), grads=[_np(g[0]) for g in piece["grads"]], dsc=_np(piece["dsc"]),
                             zeros_ok=zeros_ok, same=piece["same_as_no_grad"], launches=C.globalize(piece["call"], head0[0])))
    if dist.get_rank() != 0:
        return None
    t = lambda a: torch.as_tensor(a).to(C.dev())  # noqa: E731
    out = torch.cat([t(g["out"])[:Sl] for g in got] + [t(got[0]["out"])[Sl:]], dim=0).transpose(0, 1)  # (H, S+T, D)
    text_same = all(torch.equal(t(g["out"])[Sl:], t(got[0]["out"])[Sl:]) for g in got)
    grads = []
    for i in range(3):
        video = torch.cat([t(g["grads"][i])[:, :Sl] for g in got], dim=1)
        text = sum(t(g["grads"][i])[:, Sl:].double() for g in got)
        grads.append(torch.cat([video.double(), text], dim=1))
    dsc = sum(t(g["dsc"]).double() for g in got)
    return dict(out=out, grads=grads, dsc=dsc, zeros_ok=all(g["zeros_ok"] for g in got), text_same=text_same,
                same_as_no_grad=all(g["same"] for g in got), launches=[c for g in got for c in g["launches"]])


def _operator_worker(rank, world, port, ret, model, H, dtype_name):
    dist, SP = _setup(rank, world, port)
    dtype = DTYPES[dtype_name]
    T, te = C.text_of(model)
    q, k, v, sc, cot = C.operator_case(model, H, dtype)
    piece = _sp_operator(model, q, k, v, sc, cot, rank, world)
    from vorta_amd.attention._sp import _mixture_placement
    counts = _mixture_placement(H, world)[1]
    head0 = (sum(counts[:rank]), sum(counts[:rank + 1]))
    glob = _assemble(dist, piece, H, world, T, head0)
    if rank == 0:
        res = dict(counts=counts, zeros_ok=glob["zeros_ok"], text_same=glob["text_same"], same_as_no_grad=glob["same_as_no_grad"])
        # 1. forward: against the float64 oracle, beside the single-process operator on the same tensors
        one = C.single_process_forward(model, q, k, v, sc)[0]
        ref = torch.as_tensor(C.oracle_forward(model, q, k, v, sc)[0]).to(C.dev())
        res["fwd"] = (C.rel_err(glob["out"], ref), C.rel_err(one, ref))
        res["bits_equal"] = torch.equal(glob["out"].to(dtype), one)
        # 2. backward: float64 / 16-bit autograd of the restatement of the launches the ranks recorded
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
        ret["res"] = res
    dist.barrier()
    SP.cleanup()


def _stacked_worker(rank, world, port, ret):
    """two layers, the second fed by the first: backward through both == the layers one at a time.  A saved tensor living in
    a buffer the second layer overwrites would give the first layer another layer's q, k, v."""
    dist, SP = _setup(rank, world, port)
    from vorta_amd.routed import sp_soft_mixture_attention_autograd as op
    model, H, dtype = "hunyuan", 4, torch.bfloat16
    T, te = C.text_of(model)
    kw = dict(C.geometry_kw(), model=model, text_valid=te)
    a = [C.shard(x, rank, world) if x.dim() == 4 and x.shape[1] == H else x for x in C.operator_case(model, H, dtype, seed=5)]
    b = [C.shard(x, rank, world) if x.dim() == 4 and x.shape[1] == H else x for x in C.operator_case(model, H, dtype, seed=6)]
    c1, c2 = C.shard(a[4], rank, world, dim=1), C.shard(b[4], rank, world, dim=1)
    leaf = lambda xs: [x.clone().requires_grad_(True) for x in xs]  # noqa: E731
    # both layers in one graph
    A, B = leaf(a[:4]), leaf(b[:4])
    o1 = op(A[0], A[1], A[2], T, A[3], **kw)
    o2 = op(B[0] + 0.5 * o1.transpose(1, 2), B[1], B[2], T, B[3], **kw)
    ((o1 * c1).sum() + (o2 * c2).sum()).backward()
    both = [x.grad.clone() for x in A + B]
    # one at a time: layer 2 on the (equal) output of layer 1, then layer 1 with the cotangent layer 2 hands down
    A1 = leaf(a[:4])
    p1 = op(A1[0], A1[1], A1[2], T, A1[3], **kw)
    q2 = (b[0] + 0.5 * p1.detach().transpose(1, 2)).requires_grad_(True)
    B1 = leaf(b[1:4])
    p2 = op(q2, B1[0], B1[1], T, B1[2], **kw)
    (p2 * c2).sum().backward()
    (p1 * (c1 + 0.5 * q2.grad.transpose(1, 2))).sum().backward()
    single = [x.grad for x in A1] + [q2.grad] + [x.grad for x in B1]
    torch.cuda.synchronize()
    names = ["dq1", "dk1", "dv1", "dsc1", "dq2", "dk2", "dv2", "dsc2"]
    ret[rank] = dict(outputs_equal=torch.equal(o1, p1) and torch.equal(o2, p2),
                     errs={n: C.rel_err(x, y) for n, x, y in zip(names, both, single)},
                     equal={n: torch.equal(x, y) for n, x, y in zip(names, both, single)})
    dist.barrier()
    SP.cleanup()


def _processor_worker(rank, world, port, ret, which, dtype_name):
    """Train processor (differentiable=True) on this rank's shard; rank 0 compares the assembled gradients with the float64
    restatement of tests/test_hip_processors_grad.py (its helpers, with this module's text lengths)."""
    import test_hip_processors_grad as G
    G.T, G.TE = C.T_HY, C.TE_HY  # (this process only: a spawned worker)
    dist, SP = _setup(rank, world, port)
    dtype = DTYPES[dtype_name]
    P, Sl = world, G.S // world
    hy = which != "wan"
    if hy:
        from vorta_amd.attention import HunyuanVideoFlashAttnProcessorTripleTrain as Train
        attn = G._HyAttn(which == "hunyuan_dual", dtype, seed=31 + (which == "hunyuan_dual"))
        hidden, enc, rope, mask, score, kw = G._hy_case(dtype, 7)
        call = lambda p, h, e, sc: p(attn, h, e, mask, rope, routing_score=sc, **kw)  # noqa: E731
        restated, rope64 = G._hy_restated, rope
    else:
        from vorta_amd.attention import WanAttnProcessorTripleTrain as Train
        attn = G._WanAttn(dtype, seed=41)
        hidden, enc, freqs, rope64, score, kw = G._wan_case(dtype, 9)
        enc = None
        call = lambda p, h, e, sc: p(attn, h, None, None, freqs, routing_score=sc, **kw)  # noqa: E731
        restated = G._wan_restated
    proc = Train(differentiable=True)
    # the single-process no_grad call, before anything is sharded
    SP._enabled = False
    with torch.no_grad():
        one = call(proc, hidden, enc, score)
    SP._enabled = True
    one = one if isinstance(one, tuple) else (one,)
    h_loc = hidden[:, rank * Sl:(rank + 1) * Sl].clone().requires_grad_(True)
    leaves = {"hidden": h_loc, "routing_score": score.clone().requires_grad_(True)}
    if hy:
        leaves["enc"] = enc.clone().requires_grad_(True)
    with torch.no_grad():
        ng = call(proc, h_loc.detach(), enc, score)
    ng = ng if isinstance(ng, tuple) else (ng,)
    for p in attn.parameters():
        p.grad = None
    with C.RecordSp() as rec:
        outs = call(proc, h_loc, leaves.get("enc"), leaves["routing_score"])
    outs = outs if isinstance(outs, tuple) else (outs,)
    gen = torch.Generator(device="cpu").manual_seed(17)  # (the same cotangents on every rank; a single block has no to_out)
    cot_h = torch.randn((1, G.S, outs[0].shape[-1]), generator=gen).to(dtype).to(C.dev())
    cot_e = torch.randn((1, G.T, outs[1].shape[-1]), generator=gen).to(dtype).to(C.dev()) if hy else None
    loss = (outs[0] * cot_h[:, rank * Sl:(rank + 1) * Sl]).sum()
    if hy:
        loss = loss + (outs[1] * cot_e).sum()  # the text rows are replicated: every rank sees the same loss on them
    loss.backward()
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    # refusals that stay (6): differentiable=False under grad, the dense teacher, the dense processor
    refused = {}
    for name, fn in (("differentiable_false", lambda: call(Train(), h_loc, leaves.get("enc"), leaves["routing_score"])),
                     ("use_original_attn", lambda: proc(attn, h_loc, leaves.get("enc"), mask if hy else None,
                                                        rope if hy else freqs, use_original_attn=True,
                                                        routing_score=score, **kw)),
                     ("dense", lambda: _dense_processor(hy)(attn, h_loc, leaves.get("enc"), mask if hy else None,
                                                           rope if hy else freqs))):
        try:
            fn()
            refused[name] = False
        except NotImplementedError:
            refused[name] = True
    # the gradients: sequence shards concatenated; parameters, text-side tensors and scores summed over the ranks -- except
    # what sits BEHIND the text all-gather (to_add_out): every rank computes that gradient whole, so it is averaged
    heads = (rank * (G.H // P), (rank + 1) * (G.H // P))
    grads = {n: _np(t.grad) for n, t in leaves.items()}
    grads.update({n: _np(p.grad) for n, p in attn.named_parameters() if p.grad is not None})
    mine = torch.zeros(G.H, dtype=torch.bool)
    mine[heads[0]:heads[1]] = True
    zeros_ok = bool((leaves["routing_score"].grad[0][~mine] == 0).all())
    got = _gather(dist, dict(grads=grads, outs=[_np(o) for o in outs], ng=[_np(o) for o in ng], zeros_ok=zeros_ok,
                             launches=C.globalize(rec.calls[0], heads[0])))
    if rank == 0:
        t = lambda a: torch.as_tensor(a).to(C.dev())  # noqa: E731
        total = {}
        for n in got[0]["grads"]:
            if n == "hidden":
                total[n] = torch.cat([t(g["grads"][n]) for g in got], dim=1).double()
            else:
                total[n] = sum(t(g["grads"][n]).double() for g in got)
                if n.startswith("to_add_out"):
                    total[n] = total[n] / P
        recorded = C.as_launches([c for g in got for c in g["launches"]])
        leaves0 = {"hidden": hidden, "routing_score": score}
        if hy:
            leaves0["enc"] = enc
        cots = [cot_h] + ([cot_e] if hy else [])

        def reference(dt):
            Pm = {n: p.detach().to(dt).requires_grad_(True) for n, p in attn.named_parameters()}
            L = {n: x.detach().to(dt).requires_grad_(True) for n, x in leaves0.items()}
            o = restated(attn, Pm, L["hidden"], L.get("enc"), L["routing_score"], rope64, recorded, False)
            names = list(L) + list(Pm)
            g = torch.autograd.grad(sum((a * c.to(dt)).sum() for a, c in zip(o, cots)), [dict(L, **Pm)[n] for n in names],
                                    allow_unused=True)
            return dict(zip(names, g)), o

        r64, o64 = reference(torch.float64)
        r16, _ = reference(dtype)
        out_sp = [torch.cat([t(g["outs"][0]) for g in got], dim=1)] + ([t(got[0]["outs"][1])] if hy else [])
        ng_sp = [torch.cat([t(g["ng"][0]) for g in got], dim=1)] + ([t(got[0]["ng"][1])] if hy else [])
        res = dict(zeros_ok=all(g["zeros_ok"] for g in got), refused=refused, bwd={}, missing=[],
                   fwd=[(C.rel_err(a, r), C.rel_err(b, r)) for a, b, r in zip(ng_sp, one, o64)],
                   fwd_grad_mode=[C.rel_err(a, r) for a, r in zip(out_sp, o64)])
        for name in G.WANTED:
            if r64.get(name) is None:
                continue
            if name not in total:
                res["missing"].append(name)
                continue
            res["bwd"][name] = (C.rel_err(total[name], r64[name]), C.rel_err(r16[name], r64[name]))
        ret["res"] = res
    else:
        ret[rank] = dict(refused=refused)
    dist.barrier()
    SP.cleanup()


def _dense_processor(hy):
    from vorta_amd.attention import HunyuanVideoFlashAttnProcessor, WanAttnProcessor2_0
    return (HunyuanVideoFlashAttnProcessor if hy else WanAttnProcessor2_0)(differentiable=True)


# --------------------------------------------------------------------------------------------------------------- parent
def _run(target, world, args, limit=240):
    """spawn `world` ranks, join every one under ONE time limit; a failed or timed-out worker fails the test"""
    import torch.multiprocessing as mp
    assert world <= 4
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=target, args=(r, world, port, ret) + tuple(args)) for r in range(world)]
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


def _check(kind, case, pairs):
    """every (error, yardstick error) pair: printed and kept first, then the bound e <= 2 x yardstick"""
    for name, (e, e_y) in pairs.items():
        print(f"{kind} {case} {name}: e {e:.3e} yardstick {e_y:.3e} ratio {e / max(e_y, 1e-300):.3f}")
        FIGURES.append((kind, case, name, e, e_y))
    for name, (e, e_y) in pairs.items():
        assert e <= 2.0 * e_y, f"{kind} {case} {name}: e {e:.3e} > 2 x {e_y:.3e}"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("world,H", [(2, 4), (4, 4), (2, 3)], ids=["w2h4", "w4h4", "w2h3_uneven"])
def test_operator_forward_and_backward(world, H, model, dtype):
    """1 + 2: the assembled operator against the oracle beside the single-process operator; its gradients (video shards
    concatenated, text rows and score gradients summed over the ranks) against the restatement's float64 autograd"""
    res = _run(_operator_worker, world, (model, H, dtype))["res"]
    case = f"{model} world {world} H {H} {dtype}"
    assert res["counts"] == ([2, 1] if H == 3 else [H // world] * world)
    assert res["text_same"] and res["same_as_no_grad"]  # every rank holds the same text rows; grad form == no_grad form
    BITS[case] = res["bits_equal"]
    print(f"forward {case}: bits equal to the single-process operator: {res['bits_equal']}")
    _check("forward (SP vs one process, against the oracle)", case, {"out": res["fwd"]})
    assert res["restated_forward"] < 1.5e-2  # the restatement states this forward (tests/test_hip_processors_grad.py)
    _check("backward (kernels vs torch 16-bit autograd)", case, res["bwd"])
    assert res["zeros_ok"], "text rows / score gradients outside a rank's heads must be exactly zero"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["wan", "hunyuan_single", "hunyuan_dual"])
def test_train_processors_under_sequence_parallel(which, dtype):
    """3 + 6: TripleTrain(differentiable=True) on two ranks: gradients of hidden_states, routing_score and the projection /
    norm weights against the float64 restatement; the no_grad call against the single-process call; what keeps refusing"""
    ret = _run(_processor_worker, 2, (which, dtype))
    res = ret["res"]
    case = f"{which} world 2 {dtype}"
    assert not res["missing"], res["missing"]
    assert len(res["bwd"]) >= (8 if which != "hunyuan_dual" else 15)
    _check("processor forward, no_grad (SP vs one process, against float64)", case,
           {f"out{i}": p for i, p in enumerate(res["fwd"])})
    assert all(e < 1.5e-2 for e in res["fwd_grad_mode"])
    _check("processor backward (kernels vs torch 16-bit autograd)", case, res["bwd"])
    assert res["zeros_ok"]
    for r in (res, ret[1]):
        assert r["refused"] == {"differentiable_false": True, "use_original_attn": True, "dense": True}, r["refused"]


def test_two_stacked_layers_keep_their_saved_tensors():
    """4: forward, forward, backward through both == the layers one at a time.  The forward, dq and the score gradients are
    bit-reproducible; dk / dv are sums of float32 atomics rounded once to bf16, so two runs may differ by one ulp of
    bf16 (2^-8 relative) in some elements and by no more."""
    ret = _run(_stacked_worker, 2, ())
    for r in range(2):
        res = ret[r]
        print(r, res["errs"])
        assert res["outputs_equal"]
        for n in ("dq2", "dsc2", "dsc1"):
            assert res["equal"][n], (r, n, res["errs"][n])
        for n, e in res["errs"].items():
            assert e <= 2.0 ** -8, (r, n, e)


def test_rccl_group_of_one_rank():
    """5: forward + backward with the collectives forced through a real RCCL group of one rank (a fresh child process)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0",
               VORTA_SP_FORCE_COLLECTIVES="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rccl_single_rank_soft_mixture.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines and r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rep = json.loads(lines[-1])
    assert rep["backend"] == "nccl"
    # q, k, v in + o back (forward), d_out in + dq, dk, dv back (backward); the text all-gather
    assert rep["collective_calls"].get("all_to_all_single", 0) == 8 and rep["collective_calls"].get("all_gather", 0) == 1, rep
    _check("RCCL, one rank (SP vs the single-GPU operator, against float64)", "hunyuan H 4 bf16",
           {n: tuple(p) for n, p in rep["pairs"].items()})


def test_accuracy_summary_written():
    """the figures of this module's cases (runs after them)"""
    if not FIGURES:
        return
    lines = []
    for kind in dict.fromkeys(f[0] for f in FIGURES):
        lines.append(kind + ": error / yardstick error (bound: 2)")
        for _, case, name, e, e_y in (f for f in FIGURES if f[0] == kind):
            lines.append(f"  {case} {name}: {e:.3e} / {e_y:.3e} = {e / max(e_y, 1e-300):.3f}")
    lines.append("forward bits equal to the single-process operator:")
    lines += [f"  {case}: {'yes' if b else 'no'}" for case, b in BITS.items()]
    print("\n".join(lines))
    path = os.environ.get("VORTA_SP_SOFT_MIXTURE_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("tests/test_hip_sp_soft_mixture.py: gloo ranks sharing one MI355X (host-staged transport)\n" + "\n".join(lines) + "\n")
