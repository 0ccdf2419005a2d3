"""GPU: `routed.sampled_expert_fidelity` -- what every expert would have written on a sample of query rows -- and the launch
under it, `ops.gather_sample_rows`.

Held apart: (1) the three compact buffers against the rows of the full-size expert outputs of the soft mixture's forward
(`routed_attention(every_head_everywhere, expert_outs=...)`), bit for bit; (2) the gather alone against torch indexing; (3) the
record against a float64 evaluation of the compact buffers (the chain bound of vorta_expert_fidelity); (4) column 2 = the routed
output as launched; (5) no host read, graph replay, equal bits on every run and for host and device head lists.

Fixtures of tests/test_hip_routed_fidelity.py: latent (8,6,8), tile (2,3,4), window (3,3,3), coreset window (2,3,2), rate 0.5:
S = 384, H = 6; Hunyuan text 16 / 11 valid; the partial case (7,9,6) / tile (2,2,4), S = 378; (8,12,12), S = 1152, where the
dense launch cuts its keys."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_hip_routed_fidelity import (EXPERTS, H, D, P_LATENT, P_TILE, LATENT, TILE, T_TEXT, T_VALID, _cut_inputs, _geom, _inputs,
                                      _text, partial_on)  # noqa: F401  (partial_on: a fixture)
from _util import dev

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_FULL = {}


def _full_experts(model, latent, tile, dtype):
    """the three full-size expert outputs (H, S + T, D) of every head, computed once per case"""
    from vorta_amd.routed import HeadRouting, routed_attention
    key = (model, latent, tile, dtype)
    if key not in _FULL:
        q, k, v, _ = _inputs(model, latent, dtype)
        T, te = _text(model)
        bufs = [torch.empty_like(q) for _ in range(3)]
        routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, dev()), _geom(latent, tile), model=model, text_len=T,
                         text_valid=te, expert_outs=bufs, fp8=False)
        torch.cuda.synchronize()
        _FULL[key] = [b[0] for b in bufs]
    return _FULL[key]


def _rows_case(model, latent, tile, dtype, sizes):
    from vorta_amd.routed import sample_rows, sampled_expert_fidelity
    q, k, v, _ = _inputs(model, latent, dtype)
    T, te = _text(model)
    S = latent[0] * latent[1] * latent[2]
    full = _full_experts(model, latent, tile, dtype)
    geom = _geom(latent, tile)
    for n in sizes:
        outs = []
        sampled_expert_fidelity(q, k, v, geom, model=model, text_len=T, text_valid=te, rows=n, seed=3, outputs=outs)
        assert len(outs) == 4
        order = outs[-1]
        tokens = sample_rows(S, n, 3, dev())[order].long()
        assert sorted(order.tolist()) == list(range(n))
        for name, got, want in zip(("dense", "coreset", "sliding"), outs, full):
            same = torch.equal(got, want[:, tokens])
            bad = (got != want[:, tokens]).any(-1).nonzero().tolist()[:4]
            assert same, f"{model} {latent} {dtype} n={n}: {name} rows differ from the full-size expert at (head, position) {bad}"
    return geom


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_rows_are_the_full_size_experts_rows(model, dtype):
    """n = S visits every centre, kept margin and dropped margin; every key list is under 16 key blocks: no launch is cut"""
    _rows_case(model, LATENT, TILE, DTYPES[dtype], (384, 96))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_rows_on_a_partial_geometry(partial_on, model, dtype):
    """three key-list lengths (three sliding launches) and the remainder tokens outside the whole coreset windows"""
    geom = _rows_case(model, P_LATENT, P_TILE, DTYPES[dtype], (378, 96))
    assert geom.is_partial and geom.C > 0


def test_rows_where_the_dense_launch_cuts_its_keys():
    """S = 1152: only the dense column is cut (18 key blocks: two parts); it is held to the bound of the existing key-cut test,
    the coreset (9 blocks) and sliding (11 blocks) rows stay bit-equal"""
    import vorta_amd.routed as rt
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows, sampled_expert_fidelity
    latent, S = (8, 12, 12), 1152
    q, k, v, _ = _cut_inputs()
    geom = _geom(latent)
    assert rt.fidelity_ref_splits(S) == 2 and rt.fidelity_ref_splits(geom.S_low) == 1 and rt.fidelity_ref_splits(geom.sta_class_n_kv[0]) == 1
    bufs = [torch.empty_like(q) for _ in range(3)]
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(3, dev()), geom, model="wan", expert_outs=bufs, fp8=False)
    for n in (S, 96):
        outs = []
        fid = sampled_expert_fidelity(q, k, v, geom, model="wan", rows=n, outputs=outs)
        tokens = sample_rows(S, n, 0, dev())[outs[-1]].long()
        assert torch.equal(outs[1], bufs[1][0][:, tokens]) and torch.equal(outs[2], bufs[2][0][:, tokens])
        d = outs[0].double() - bufs[0][0][:, tokens].double()
        rel = torch.sqrt((d * d).sum((1, 2)) / (bufs[0][0][:, tokens].double() ** 2).sum((1, 2)))
        print(f"n = {n}: dense rows, keys cut in two against whole: rel_error {rel.tolist()}")
        assert bool((rel < 2.0 ** -7).all())
        assert bool(torch.isfinite(fid.sq_err[:, :2]).all()) and bool(torch.isnan(fid.sq_err[:, 2]).all())


# ---- (2) the gather alone ------------------------------------------------------------------------------------------------

def _gather_case(dtype, n, seed=5):
    gen = torch.Generator().manual_seed(seed)
    Hh, N, G, n_dup = 5, 300, 20, 5
    wide = torch.randn((Hh, N, 2 * D + 8), generator=gen).to(dtype).to(dev())
    q = wide[:, 3:, 8:8 + D]            # an offset view with a row stride of 264 elements
    out = torch.randn((Hh, N - 3, D), generator=gen).to(dtype).to(dev())
    rows = torch.randperm(N - 3, generator=gen)[:n].to(torch.int32).to(dev())
    win = torch.randint(-1, G, (n,), generator=gen).to(torch.int32).to(dev())
    keep = torch.randint(0, N - 3, (Hh, G + 7), generator=gen).to(torch.int32).to(dev())
    drop = torch.randint(0, N - 3, (Hh, G, n_dup), generator=gen).to(torch.int32)
    # make the dropped case common: half the positions with a window are written into a slot's drop list
    for y in range(Hh):
        for p in range(0, n, 2):
            if int(win[p]) >= 0:
                drop[y, int(win[p]), (p + y) % n_dup] = int(rows[p])
    return q, out, rows, win, keep, drop.to(dev())


def _gather_want(q, out, rows, win, keep, drop, heads):
    n = rows.numel()
    want = [torch.full((q.shape[0], n, D), 7.0, dtype=q.dtype, device=q.device) for _ in range(3)]
    rows_h, win_h, keep_h, drop_h = (t.cpu().tolist() for t in (rows, win, keep, drop))
    for y, h in enumerate(heads):
        rep = [keep_h[y][w] if w >= 0 and r in drop_h[y][w] else r for r, w in zip(rows_h, win_h)]
        rep = torch.tensor(rep, dtype=torch.int64, device=q.device)
        want[0][h], want[1][h], want[2][h] = q[h][rows.long()], q[h][rep], out[h][rows.long()]
    return want


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("n", [0, 1, 33, 257])
def test_gather_against_torch_indexing(dtype, n):
    from vorta_amd import ops
    q, out, rows, win, keep, drop = _gather_case(DTYPES[dtype], n)
    Hh = q.shape[0]
    cases = [(None, None, None, list(range(Hh))),
             (torch.tensor([3, 0, 4], dtype=torch.int32, device=dev()), None, None, [3, 0, 4]),
             (torch.tensor([2, 4, 1, 0, 3], dtype=torch.int32, device=dev()), 5, torch.tensor([2], dtype=torch.int32, device=dev()),
              [2, 4])]
    for head_list, n_heads, n_dev, heads in cases:
        # destinations are views inside a larger sentinel-filled storage: rows past n and the storage around them stay
        store = [torch.full((Hh + 1, n + 3, D + 8), 7.0, dtype=q.dtype, device=dev()) for _ in range(3)]
        dst = [s[:Hh, 1:n + 1, 8:] for s in store]
        ops.gather_sample_rows(q, rows, dst_q=dst[0], dst_qrep=dst[1], dst_out=dst[2], out=out, win=win, keep_rows=keep,
                               drop_rows=drop, head_list=head_list, n_heads=n_heads, n_heads_dev=n_dev)
        torch.cuda.synchronize()
        want = _gather_want(q, out, rows, win, keep, drop, heads)
        for i, name in enumerate(("dst_q", "dst_qrep", "dst_out")):
            assert torch.equal(dst[i], want[i]), (name, heads)
            outside = store[i].clone()
            outside[:Hh, 1:n + 1, 8:] = 7.0
            assert bool((outside == 7.0).all()), f"{name}: storage outside the destination was written"
        if n >= 33 and heads == list(range(Hh)):
            assert not torch.equal(want[0], want[1]), "the case must hold dropped rows"
    # one destination only: the others' sources and tables need not be given
    only = torch.full((Hh, n, D), 7.0, dtype=q.dtype, device=dev())
    ops.gather_sample_rows(q, rows, dst_q=only)
    assert torch.equal(only, q[:, rows.long()])
    # all windows -1: the representative is the row itself
    rep = torch.full((Hh, n, D), 7.0, dtype=q.dtype, device=dev())
    ops.gather_sample_rows(q, rows, dst_qrep=rep, win=torch.full_like(win, -1), keep_rows=keep, drop_rows=drop)
    assert torch.equal(rep, q[:, rows.long()])


def test_gather_error_codes_with_nothing_launched():
    from vorta_amd import _C
    Hh, n, N = 2, 16, 20
    q = torch.randn((Hh, N, D), device=dev()).half()
    out = torch.randn((Hh, N, D), device=dev()).half()
    dst = [torch.full((Hh, n, D), 7.0, dtype=torch.float16, device=dev()) for _ in range(3)]
    rows = torch.arange(n, dtype=torch.int32, device=dev())
    win = torch.zeros(n, dtype=torch.int32, device=dev())
    keep = torch.zeros((Hh, 4), dtype=torch.int32, device=dev())
    drop = torch.zeros((Hh, 1, 3), dtype=torch.int32, device=dev())
    lst = torch.arange(Hh + 1, dtype=torch.int32, device=dev())
    lib, stream = _C.lib(), torch.cuda.current_stream().cuda_stream
    ten = lambda t: _C.Tensor(t.data_ptr(), t.stride(0), t.stride(1))  # noqa: E731
    odd = lambda t: _C.Tensor(t.data_ptr() + 2, t.stride(0), t.stride(1))  # noqa: E731
    null = _C.Tensor(None, 0, 128)

    def args(**over):
        a = _C.GatherSampleRowsArgs()
        a.struct_size = C.sizeof(_C.GatherSampleRowsArgs)
        a.dtype, a.head_dim, a.n_heads, a.n_rows, a.n_dup = _C.VORTA_FP16, 128, Hh, n, 3
        a.q, a.out, a.dst_q, a.dst_qrep, a.dst_out = ten(q), ten(out), ten(dst[0]), ten(dst[1]), ten(dst[2])
        a.rows, a.win = rows.data_ptr(), win.data_ptr()
        a.keep_rows, a.keep_rows_stride_h, a.drop_rows, a.drop_rows_stride_h = keep.data_ptr(), 4, drop.data_ptr(), 3
        for key, val in over.items():
            setattr(a, key, val)
        return a

    EINVAL, EUNSUP = _C.VORTA_EINVAL, _C.VORTA_EUNSUPPORTED
    bad = [("struct_size", dict(struct_size=8), EINVAL), ("dtype fp32", dict(dtype=_C.VORTA_FP32), EUNSUP),
           ("dtype e4m3", dict(dtype=_C.VORTA_FP8E4M3), EUNSUP), ("head_dim 64", dict(head_dim=64), EUNSUP),
           ("negative heads", dict(n_heads=-1), EINVAL), ("negative rows", dict(n_rows=-1), EINVAL),
           ("negative n_dup", dict(n_dup=-1), EINVAL), ("too many slots", dict(n_heads=65536), EINVAL),
           ("null rows", dict(rows=None), EINVAL), ("misaligned rows", dict(rows=rows.data_ptr() + 2), EINVAL),
           ("null win", dict(win=None), EINVAL), ("misaligned win", dict(win=win.data_ptr() + 1), EINVAL),
           ("null keep", dict(keep_rows=None), EINVAL), ("null drop", dict(drop_rows=None), EINVAL),
           ("misaligned head_list", dict(head_list=lst.data_ptr() + 2), EINVAL),
           ("misaligned n_heads_dev", dict(n_heads_dev=lst.data_ptr() + 1), EINVAL),
           ("null q", dict(q=null), EINVAL), ("null out", dict(out=null), EINVAL),
           ("misaligned q", dict(q=odd(q)), EINVAL), ("misaligned dst", dict(dst_qrep=odd(dst[1])), EINVAL),
           ("odd row stride", dict(out=_C.Tensor(out.data_ptr(), out.stride(0), 129)), EINVAL),
           ("odd head stride", dict(dst_q=_C.Tensor(dst[0].data_ptr(), n * 128 + 4, 128)), EINVAL)]
    for what, over, code in bad:
        assert lib.vorta_gather_sample_rows(C.byref(args(**over)), stream) == code, what
    assert lib.vorta_gather_sample_rows(None, stream) == EINVAL
    assert lib.vorta_gather_sample_rows(C.byref(args(n_heads=0, dtype=_C.VORTA_FP32)), stream) == EUNSUP  # looked at first
    assert lib.vorta_gather_sample_rows(C.byref(args(n_heads=0)), stream) == _C.VORTA_OK
    assert lib.vorta_gather_sample_rows(C.byref(args(n_rows=0, rows=None, q=null, out=null)), stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert all(bool((d == 7.0).all()) for d in dst)
    assert lib.vorta_gather_sample_rows_args_size() == C.sizeof(_C.GatherSampleRowsArgs)
    assert lib.vorta_gather_sample_rows(C.byref(args()), stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert torch.equal(dst[0], q[:, :n]) and torch.equal(dst[2], out[:, :n])


# ---- (3) the statistics -----------------------------------------------------------------------------------------------------

def _check_record(fid, outs, heads, with_out, case):
    """the record against a float64 evaluation of the compact buffers: sums within VORTA_FIDELITY_CHAIN(n) 2^-24 relative, maxima
    exact (the float32 rounding of a difference is monotone), NaN for the heads not measured"""
    from vorta_amd import _C
    x0 = outs[0].double().cpu().numpy()
    n = x0.shape[1]
    bound = _C.fidelity_chain(n) * U
    cols = [outs[1], outs[2]] + ([outs[3]] if with_out else [])
    measured = np.zeros(H, dtype=bool)
    measured[list(heads)] = True
    got = {name: getattr(fid, name).double().cpu().numpy() for name in ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err")}
    for name, g in got.items():
        assert np.isnan(g[~measured]).all(), (case, name, "an unmeasured head is not NaN")
    worst = 0.0
    for h in heads:
        a = x0[h].reshape(-1)
        want = (a * a).sum()
        worst = max(worst, abs(got["sq_ref"][h] - want) / (bound * want))
        assert got["max_ref"][h] == np.float32(np.abs(a).max()) and got["range_ref"][h] == np.float32(a.max() - a.min())
        for j, t in enumerate(cols):
            d = t[h].double().cpu().numpy() - x0[h]
            want = (d * d).sum()
            if want == 0:
                assert got["sq_err"][h, j] == 0 and got["max_err"][h, j] == 0
                continue
            worst = max(worst, abs(got["sq_err"][h, j] - want) / (bound * want))
            assert got["max_err"][h, j] == np.float32(np.abs(d).max()), (case, h, j)
        if not with_out:
            assert np.isnan(got["sq_err"][h, 2]) and np.isnan(got["max_err"][h, 2])
    print(f"{case}: n {n} chain {_C.fidelity_chain(n)} bound {bound:.3e} largest error / bound {worst:.4f}")
    assert worst <= 1.0, (case, worst)
    assert fid.n == n * D


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_statistics_against_float64(model):
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows, sampled_expert_fidelity
    q, k, v, _ = _inputs(model)
    T, te = _text(model)
    geom, S = _geom(), 384
    kw = dict(model=model, text_len=T, text_valid=te)
    for n in (96, S):
        table = sample_rows(S, n, 0, dev())
        outs = []
        fid = sampled_expert_fidelity(q, k, v, geom, rows=table, outputs=outs, **kw)
        _check_record(fid, outs, range(H), False, f"{model} n = {n} every head")
        rel = fid.rel_error()
        assert bool((rel[:, :2] > 0).all()) and bool(torch.isnan(rel[:, 2]).all())
        # max_ref is the SampledFidelity record's: the same reference rows
        sink = []
        routed_attention(q, k, v, HeadRouting.from_expert_ids(EXPERTS, dev()), geom, fp8="native", fidelity=sink,
                         fidelity_rows=table, fidelity_heads="all", **kw)
        assert torch.equal(fid.max_ref, sink[0].max_ref) and torch.equal(fid.range_ref, sink[0].range_ref)
    # a head list: the heads it does not name hold NaN, the others the bits of the all-heads record
    outs = []
    part = sampled_expert_fidelity(q, k, v, geom, rows=table, heads=[4, 1], outputs=outs, **kw)
    _check_record(part, outs, (1, 4), False, f"{model} heads 4, 1")
    for name in ("sq_ref", "max_ref", "sq_err", "max_err"):
        assert torch.equal(getattr(part, name)[[1, 4]][..., :2], getattr(fid, name)[[1, 4]][..., :2]), name  # (column 2: NaN)
    none = sampled_expert_fidelity(q, k, v, geom, rows=table, heads=[], **kw)
    assert all(bool(torch.isnan(getattr(none, name)).all()) for name in ("sq_ref", "max_ref", "sq_err", "max_err"))
    with pytest.raises(ValueError):
        sampled_expert_fidelity(q, k, v, geom, rows=S + 1, **kw)


# ---- (4) column 2: the routed output as launched --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_column_two_is_the_routed_output(model, dtype):
    from vorta_amd.routed import HeadRouting, routed_attention
    q, k, v, _ = _inputs(model, dtype=DTYPES[dtype])
    T, te = _text(model)
    geom, routing = _geom(), HeadRouting.from_expert_ids(EXPERTS, dev())
    kw = dict(model=model, text_len=T, text_valid=te, fp8="native")
    plain = routed_attention(q, k, v, routing, geom, **kw)
    for n in (96, 384):
        sink, both = [], []
        out = routed_attention(q, k, v, routing, geom, expert_fidelity=sink, fidelity_rows=n, **kw)
        assert torch.equal(out, plain), "a sink must not change the routed output"
        assert len(sink) == 1
        fid = sink[0]
        for h, e in enumerate(EXPERTS):
            if e == 0:
                assert float(fid.sq_err[h, 2]) == 0.0 and float(fid.max_err[h, 2]) == 0.0, (h, fid.sq_err[h].tolist())
            else:
                assert float(fid.sq_err[h, 2]) == float(fid.sq_err[h, e - 1]) > 0, (h, fid.sq_err[h].tolist())
                assert float(fid.max_err[h, 2]) == float(fid.max_err[h, e - 1])
        # both sinks at once share the sample
        out = routed_attention(q, k, v, routing, geom, expert_fidelity=both, fidelity=sink, fidelity_rows=n, fidelity_heads="all", **kw)
        assert torch.equal(out, plain) and torch.equal(both[0].sq_err, fid.sq_err)
        assert torch.equal(both[0].max_ref, sink[-1].max_ref)
    with pytest.raises(ValueError):
        routed_attention(q, k, v, routing, geom, expert_fidelity=[], expert_outs=[torch.empty_like(q) for _ in range(3)], **kw)


# ---- (5) execution --------------------------------------------------------------------------------------------------------------

NAMES = ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err")


def _same(a, b):
    for name in NAMES:
        assert np.array_equal(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy(), equal_nan=True), name


def test_device_lists_give_the_same_bits_without_a_host_read():
    from vorta_amd.routed import sample_rows, sampled_expert_fidelity
    q, k, v, _ = _inputs("hunyuan")
    geom = _geom()
    table = sample_rows(384, 96, 0, dev())
    out = torch.randn(q.shape, device=dev()).to(q.dtype)
    keep = out.clone()
    host = torch.tensor([5, 0, 2, 3], dtype=torch.int32, device=dev())
    slots = torch.tensor([5, 0, 2, 3, 1, 4], dtype=torch.int32, device=dev())
    count = torch.tensor([4], dtype=torch.int32, device=dev())
    kw = dict(model="hunyuan", text_len=T_TEXT, text_valid=T_VALID, rows=table, out=out)
    a = sampled_expert_fidelity(q, k, v, geom, heads=host, **kw)
    sampled_expert_fidelity(q, k, v, geom, heads=(slots, count), **kw)  # (warm: tables, allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
    try:
        b = sampled_expert_fidelity(q, k, v, geom, heads=(slots, count), **kw)
        c = sampled_expert_fidelity(q, k, v, geom, heads=host, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same(a, b)
    _same(a, c)
    assert torch.isfinite(a.sq_err).all(1).nonzero().flatten().tolist() == [0, 2, 3, 5]
    assert torch.equal(out, keep), "`out` is only read"


def test_graph_replay_reports_the_new_inputs():
    from vorta_amd.routed import sample_rows, sampled_expert_fidelity
    qa, ka, va, _ = _inputs("wan")
    geom = _geom()
    table = sample_rows(384, 96, 0, dev())
    gen = torch.Generator().manual_seed(99)
    qb, kb, vb = (torch.randn(qa.shape, generator=gen).to(qa.dtype).to(dev()) for _ in range(3))
    q, k, v = (x.clone() for x in (qa, ka, va))
    kw = dict(model="wan", rows=table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        sampled_expert_fidelity(q, k, v, geom, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec = sampled_expert_fidelity(q, k, v, geom, **kw)
    for src in ((qa, ka, va), (qb, kb, vb)):
        for dst, s in zip((q, k, v), src):
            dst.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        eager = sampled_expert_fidelity(*src, geom, **kw)
        _same(rec, eager)
        again = sampled_expert_fidelity(*src, geom, **kw)  # two runs: equal bits
        _same(eager, again)
    assert not torch.equal(rec.sq_ref, sampled_expert_fidelity(qa, ka, va, geom, **kw).sq_ref)
