"""GPU: `routed_attention(..., fidelity=[...])` -- the routed output as run against dense attention on sampled query rows.

Three things are held apart.  (1) `out` with a sink is bit-equal to `out` without one.  (2) The reference rows the operator
computes (seen through a spy on ops.sampled_fidelity) against the oracle's dense attention on the sampled rows, at the tolerance
tests/test_hip_attention.py holds the dense launch to.  (3) The reported statistics against the float64 restatement applied to
the read-back `ref` and `out` (tests/_sampled_fidelity_restate.py: the chain bound): the gather, the row tables, the head
lists and the compare.  Exactly the heads the mode names are finite; every other head is NaN.

Geometry of the fixtures: latent (8,6,8), tile (2,3,4), window (3,3,3), coreset window (2,3,2): S = 384, H = 6, D = 128,
Hunyuan text 16 / 11 valid; the partial case is latent (7,9,6), tile (2,2,4) with set_partial_geometry(True) (S = 378).
n = 48 sampled rows (strata of 8 tokens: a stratum is narrower than a tile row), and n = S on Wan."""
import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O
from _sampled_fidelity_restate import NAMES, check as check_stats
from _util import check as check_dense, dev

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, GROUP = (8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)
P_LATENT, P_TILE = (7, 9, 6), (2, 2, 4)
H, D, T_TEXT, T_VALID = 6, 128, 16, 11
EXPERTS = [0, 1, 2, 0, 1, 2]
N = 48
PRECISIONS = ("native", "i8pv", "fp8pv", "auto8")
_CACHE = {}


@pytest.fixture()
def partial_on():
    from vorta_amd import _partial
    before = _partial._partial_geometry
    _partial.set_partial_geometry(True)
    yield
    _partial._partial_geometry = before


def _text(model):
    return (T_TEXT, T_VALID) if model == "hunyuan" else (0, 0)


def _inputs(model, latent=LATENT, dtype=torch.bfloat16):
    """q, k, v (1, H, S + T, D) on the device and the oracle's dense attention of every head (float64), computed once"""
    key = (model, latent, dtype)
    if key not in _CACHE:
        S, (T, te) = latent[0] * latent[1] * latent[2], _text(model)
        gen = torch.Generator().manual_seed(1234 + len(model) + S)
        q, k, v = (torch.randn((1, H, S + T, D), generator=gen).to(dtype) for _ in range(3))
        dense = O.dense_attention(q[0].double().numpy(), k[0].double().numpy(), v[0].double().numpy(), kv_valid=S + te,
                                  q_valid=S + te)
        _CACHE[key] = tuple(x.to(dev()) for x in (q, k, v)) + (dense,)
    return _CACHE[key]


def _geom(latent=LATENT, tile=TILE, row_map=None):
    from vorta_amd.routed import geometry_for
    return geometry_for(latent, tile, WINDOW, GROUP, 0.5, dev(), row_map=row_map)


class Spy:
    """records what ops.sampled_fidelity was handed: (ref, out, rows, the head list as launched)"""

    def __init__(self, monkeypatch):
        from vorta_amd import ops
        self.calls, self.real = [], getattr(ops.sampled_fidelity, "real", ops.sampled_fidelity)  # (never a spy on a spy)
        monkeypatch.setattr(ops, "sampled_fidelity", self)

    def __call__(self, ref, out, rows, head_list=None, n_heads=None, n_heads_dev=None, **kw):
        self.calls.append((ref, out, rows, head_list, n_heads, n_heads_dev))
        return self.real(ref, out, rows, head_list=head_list, n_heads=n_heads, n_heads_dev=n_heads_dev, **kw)


def _measured(experts, mode, split=()):
    return [h for h, e in enumerate(experts) if (e in (1, 2) or mode == "all") and h not in split]


def _verify(rec, spy, experts, mode, tokens, dense, dtype, split=(), case=""):
    """the record of one call against the spy's tensors, the oracle and the restatement"""
    heads = _measured(experts, mode, split)
    ref, out, rows = spy.calls[-1][:3]
    assert all(c[0] is ref and c[2] is rows for c in spy.calls)  # one reference buffer, one table, a launch per expert
    assert torch.equal(rec.rows, tokens) and rec.n == tokens.numel() * D
    assert rec.expert.dtype == torch.int32 and rec.expert.is_cuda and rec.expert.tolist() == list(experts)
    for h in heads:  # (2) the reference rows
        check_dense(ref[h], dense[h][tokens.cpu().numpy()], dtype)
    check_stats(rec, ref, out, rows, heads=heads, case=case)  # (3): also that every other head is NaN
    finite = torch.isfinite(rec.sq_err)
    assert finite.nonzero().flatten().tolist() == heads and int((~finite).sum()) == H - len(heads)
    assert int(torch.isnan(rec.rel_error()).sum()) == H - len(heads)
    return ref, out, rows


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_sink_leaves_out_alone_and_reports_the_routed_rows(monkeypatch, model, precision):
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows
    dtype = torch.bfloat16
    q, k, v, dense = _inputs(model)
    S, (T, te) = q.shape[2] - _text(model)[0], _text(model)
    geom, routing = _geom(), HeadRouting.from_expert_ids(EXPERTS, dev())
    kw = dict(model=model, text_len=T, text_valid=te, fp8=precision)
    plain = routed_attention(q, k, v, routing, geom, **kw)
    tokens = sample_rows(S, N, 0, dev())
    for mode in ("sparse", "all"):
        spy, sink = Spy(monkeypatch), []
        out = routed_attention(q, k, v, routing, geom, fidelity=sink, fidelity_rows=N, fidelity_heads=mode, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, plain), "a sink must not change the routed output"
        assert len(sink) == 1 and len(spy.calls) == (2 if mode == "sparse" else 3)
        rec = sink[0]
        _verify(rec, spy, EXPERTS, mode, tokens, dense, dtype, case=f"{model} {precision} {mode}")
        rel = rec.rel_error()
        print(f"{model} {precision} {mode}: rel_error per head {[round(float(x), 5) for x in rel.tolist()]}")
        assert bool((rel[[1, 2, 4, 5]] > 0).all())  # a sparse expert is not dense attention
        if mode == "all" and precision == "native":
            assert bool((rel[[0, 3]] < 2.0 ** -7).all()), rel  # a full head in the input dtype: the dense kernel twice
            print(f"{model} native expert-0 heads: sq_err {rec.sq_err[[0, 3]].tolist()} (zero = the same bits)")
    # an explicit table, and the default sample size (min(2048, S) = S)
    sink = []
    routed_attention(q, k, v, routing, geom, fidelity=sink, fidelity_rows=sample_rows(S, N, 7, dev()), **kw)
    assert torch.equal(sink[0].rows, sample_rows(S, N, 7, dev())) and not torch.equal(sink[0].rows, tokens)
    sink = []
    routed_attention(q, k, v, routing, geom, fidelity=sink, **kw)
    assert sink[0].rows.tolist() == list(range(S))
    with pytest.raises(ValueError):
        routed_attention(q, k, v, routing, geom, fidelity=[], fidelity_heads="dense", **kw)
    with pytest.raises(ValueError):
        routed_attention(q, k, v, routing, geom, fidelity=[], expert_outs=[torch.empty_like(q) for _ in range(3)], **kw)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_partial_geometry(monkeypatch, partial_on, model, precision):
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows
    q, k, v, dense = _inputs(model, P_LATENT)
    S, (T, te) = q.shape[2] - _text(model)[0], _text(model)
    geom = _geom(P_LATENT, P_TILE)
    assert geom.is_partial
    routing = HeadRouting.from_expert_ids(EXPERTS, dev())
    kw = dict(model=model, text_len=T, text_valid=te, fp8=precision)
    plain = routed_attention(q, k, v, routing, geom, **kw)
    spy, sink = Spy(monkeypatch), []
    out = routed_attention(q, k, v, routing, geom, fidelity=sink, fidelity_rows=N, fidelity_heads="all", **kw)
    assert torch.equal(out, plain)
    _verify(sink[0], spy, EXPERTS, "all", sample_rows(S, N, 0, dev()), dense, torch.bfloat16, case=f"partial {model} {precision}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_heads_split_by_query_range_are_never_measured(monkeypatch, dtype):
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows
    q, k, v, dense = _inputs("hunyuan", dtype=dtype)
    S, T, te = 384, T_TEXT, T_VALID
    routing = HeadRouting.from_expert_ids(EXPERTS, dev(), q_ranges={3: (128, 384)})
    for mode in ("sparse", "all"):
        spy, sink = Spy(monkeypatch), []
        routed_attention(q, k, v, routing, _geom(), model="hunyuan", text_len=T, text_valid=te, fidelity=sink,
                         fidelity_rows=N, fidelity_heads=mode, fp8="native")
        _verify(sink[0], spy, EXPERTS, mode, sample_rows(S, N, 0, dev()), dense, dtype, split=(3,), case=f"split {mode}")
    # no measured head at all: one record, every statistic NaN
    sink = []
    routed_attention(q, k, v, HeadRouting.from_expert_ids([0] * H, dev()), _geom(), model="hunyuan", text_len=T,
                     text_valid=te, fidelity=sink, fidelity_rows=N, fp8="native")
    assert len(sink) == 1 and all(bool(torch.isnan(getattr(sink[0], name)).all()) for name in NAMES)


@pytest.mark.parametrize("precision", ["native", "auto8"])
def test_device_lists_give_the_same_bits_without_a_host_read(precision):
    from vorta_amd.routed import HeadRouting, routed_attention
    q, k, v, _ = _inputs("hunyuan")
    host = HeadRouting.from_expert_ids(EXPERTS, dev())
    device = HeadRouting.from_device(host.lists, torch.tensor(host.counts_host, dtype=torch.int32, device=dev()))
    geom = _geom()
    geom.prebuild(T_VALID)
    kw = dict(model="hunyuan", text_len=T_TEXT, text_valid=T_VALID, fp8=precision, fidelity_rows=N, fidelity_heads="all")
    a = []
    out_a = routed_attention(q, k, v, host, geom, fidelity=a, **kw)
    b = []
    routed_attention(q, k, v, device, geom, fidelity=b, **kw)  # (warm: tables, sample, allocator)
    torch.cuda.synchronize()
    b = []
    torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
    try:
        out_b = routed_attention(q, k, v, device, geom, fidelity=b, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out_a, out_b)
    for name in NAMES:
        assert torch.equal(getattr(a[0], name), getattr(b[0], name)), name
    assert a[0].expert.tolist() == b[0].expert.tolist() == EXPERTS
    assert bool(torch.isfinite(b[0].sq_err).all())


def test_graph_replay_reports_the_new_routes():
    """captured with device lists; the routes change in place; a replay reports what an eager call on the new routes does"""
    from vorta_amd.routed import HeadRouting, routed_attention
    q, k, v, _ = _inputs("wan")
    geom = _geom()
    geom.prebuild(0)
    first, second = [0, 1, 2, 0, 1, 2], [2, 2, 1, 1, 0, 1]
    ha, hb = (HeadRouting.from_expert_ids(e, dev()) for e in (first, second))
    lists = ha.lists.clone()
    counts = torch.tensor(ha.counts_host, dtype=torch.int32, device=dev())
    kw = dict(model="wan", fp8="native", fidelity_rows=N)
    out = torch.empty_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        routed_attention(q, k, v, HeadRouting.from_device(lists, counts), geom, out=out, fidelity=[], **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph, sink = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph):
        routed_attention(q, k, v, HeadRouting.from_device(lists, counts), geom, out=out, fidelity=sink, **kw)
    for experts, host in ((first, ha), (second, hb)):
        lists.copy_(host.lists)
        counts.copy_(torch.tensor(host.counts_host, dtype=torch.int32, device=dev()))
        graph.replay()
        torch.cuda.synchronize()
        eager = []
        want = routed_attention(q, k, v, host, geom, fidelity=eager, **kw)
        assert torch.equal(out, want)
        for name in NAMES:
            assert np.array_equal(getattr(sink[0], name).cpu().numpy(), getattr(eager[0], name).cpu().numpy(), equal_nan=True), name
        assert sink[0].expert.tolist() == experts
        assert torch.isfinite(sink[0].sq_err).nonzero().flatten().tolist() == [h for h, e in enumerate(experts) if e]


def _cut_inputs():
    """latent (8,12,12), S = 1152, 3 heads on experts 0 / 1 / 2: 18 key blocks of 64, the smallest count at which the reference
    launch cuts its keys (routed.fidelity_ref_splits: two parts + the merge kernel)"""
    if "cut" not in _CACHE:
        S = 8 * 12 * 12
        gen = torch.Generator().manual_seed(77)
        q, k, v = (torch.randn((1, 3, S, D), generator=gen).to(torch.bfloat16) for _ in range(3))
        dense = O.dense_attention(q[0].double().numpy(), k[0].double().numpy(), v[0].double().numpy())
        _CACHE["cut"] = tuple(x.to(dev()) for x in (q, k, v)) + (dense,)
    return _CACHE["cut"]


def _watch_ref_splits(monkeypatch):
    """the n_splits of every reference launch (ops.attn_fwd calls tagged "fidelity_ref"), in launch order"""
    from vorta_amd import ops
    seen, stock = [], ops.attn_fwd
    monkeypatch.setattr(ops, "attn_fwd", lambda *a, **kw: (seen.append(kw.get("n_splits", 1)) if kw.get("tag") == "fidelity_ref"
                                                            else None, stock(*a, **kw))[1])
    return seen


def test_the_key_cut_follows_from_the_key_count_alone():
    """no launch: the parts of the reference launch are a function of n_kv -- not of n, the heads or the list form"""
    import inspect
    import vorta_amd.routed as rt
    assert rt.FIDELITY_REF_SPLITS == 8 and list(inspect.signature(rt.fidelity_ref_splits).parameters) == ["n_kv"]
    assert [rt.fidelity_ref_splits(n) for n in (1, 384, 400, 960, 961, 1152, 4032, 4033, 8320, 75600, 118896)] == \
        [1, 1, 1, 1, 2, 2, 7, 8, 8, 8, 8]


def test_reference_launch_with_split_keys(monkeypatch):
    """S = 1152: the reference rows with their keys cut in two against the oracle, the statistics against the restatement, and
    the whole-key form beside it"""
    import vorta_amd.routed as rt
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows
    latent, experts = (8, 12, 12), [0, 1, 2]
    S = 8 * 12 * 12
    assert rt.fidelity_ref_splits(S) == 2
    q, k, v, dense = _cut_inputs()
    geom, routing = _geom(latent), HeadRouting.from_expert_ids(experts, dev())
    tokens = sample_rows(S, N, 0, dev())
    seen = _watch_ref_splits(monkeypatch)
    records = {}
    for splits in (8, 1):
        monkeypatch.setattr(rt, "FIDELITY_REF_SPLITS", splits)
        spy, sink = Spy(monkeypatch), []
        routed_attention(q, k, v, routing, geom, model="wan", fp8="native", fidelity=sink, fidelity_rows=N, fidelity_heads="all")
        ref, out, rows = spy.calls[-1][:3]
        for h in range(3):
            check_dense(ref[h], dense[h][tokens.cpu().numpy()], torch.bfloat16)
        check_stats(sink[0], ref, out, rows, case=f"split keys {splits}")
        records[splits] = sink[0]
    assert seen == [2, 2, 2, 1, 1, 1]
    rel = {s: r.rel_error() for s, r in records.items()}
    print(f"expert-0 head, keys cut / whole: rel_error {float(rel[8][0]):.3e} / {float(rel[1][0]):.3e}")
    assert rel[8][0] < 2.0 ** -7 and rel[1][0] < 2.0 ** -7
    assert torch.allclose(rel[8][1:], rel[1][1:], rtol=2.0 ** -6)  # the sparse heads' errors do not hinge on the order


@pytest.mark.parametrize("n", [N, 300])
def test_device_lists_give_the_same_bits_where_the_keys_are_cut(monkeypatch, n):
    """S = 1152, where the reference launch cuts its keys: host lists (a launch of ONE head slot per expert) and device lists
    (three slots, a device count of one) cut them alike, so the records are equal bit for bit -- the expert-0 head's too, whose
    error is nothing but the summation order; n = 300 is a second query block"""
    from vorta_amd.routed import HeadRouting, routed_attention
    q, k, v, _ = _cut_inputs()
    host = HeadRouting.from_expert_ids([0, 1, 2], dev())
    device = HeadRouting.from_device(host.lists, torch.tensor(host.counts_host, dtype=torch.int32, device=dev()))
    assert host.slot_args(1, 3)["n_heads"] == 1 and device.slot_args(1, 3)["n_heads"] == 3
    geom = _geom((8, 12, 12))
    seen = _watch_ref_splits(monkeypatch)
    kw = dict(model="wan", fp8="native", fidelity_rows=n, fidelity_heads="all")
    a, b = [], []
    routed_attention(q, k, v, host, geom, fidelity=a, **kw)
    routed_attention(q, k, v, device, geom, fidelity=b, **kw)
    torch.cuda.synchronize()
    assert seen == [2] * 6
    for name in NAMES:
        print(name, getattr(a[0], name).tolist(), getattr(b[0], name).tolist())
        assert torch.equal(getattr(a[0], name), getattr(b[0], name)), name
    assert bool(torch.isfinite(b[0].sq_err).all()) and a[0].expert.tolist() == b[0].expert.tolist() == [0, 1, 2]


def test_every_row_on_wan(monkeypatch):
    """n == S: the table is the identity and the statistics are those of the whole video"""
    from vorta_amd.routed import HeadRouting, routed_attention
    q, k, v, dense = _inputs("wan")
    S = 384
    spy, sink = Spy(monkeypatch), []
    out = routed_attention(q, k, v, HeadRouting.from_expert_ids(EXPERTS, dev()), _geom(), model="wan", fp8="native",
                           fidelity=sink, fidelity_rows=S, fidelity_heads="all")
    tokens = torch.arange(S, dtype=torch.int32, device=dev())
    ref, seen, rows = _verify(sink[0], spy, EXPERTS, "all", tokens, dense, torch.bfloat16, case="wan n = S")
    assert torch.equal(rows, tokens)
    d = out[0].double() - ref.double()
    want = (d * d).sum((1, 2))
    assert torch.allclose(sink[0].sq_err.double(), want, rtol=1e-5, atol=0)


def test_a_row_map_composes_with_the_sample(monkeypatch):
    """the zero-copy sequence-parallel layout in one process: token i lives in row rm[i]; the statistics are those of the plain
    layout, bit for bit, and the table the compare saw is rm[tokens]"""
    from vorta_amd.routed import HeadRouting, routed_attention, sample_rows
    q, k, v, _ = _inputs("hunyuan")
    S, T, te = 384, T_TEXT, T_VALID
    rm = (torch.arange(S + T) * 2 + 1).to(torch.int32).to(dev())
    wide = [torch.zeros((1, H, 2 * (S + T) + 1, D), dtype=q.dtype, device=dev()) for _ in range(3)]
    for w, x in zip(wide, (q, k, v)):
        w[:, :, rm.long()] = x
    routing = HeadRouting.from_expert_ids(EXPERTS, dev())
    kw = dict(model="hunyuan", text_len=T, text_valid=te, fp8="native", fidelity_rows=N, fidelity_heads="all")
    plain = []
    out = routed_attention(q, k, v, routing, _geom(), fidelity=plain, **kw)
    spy, mapped = Spy(monkeypatch), []
    out_w = routed_attention(*wide, routing, _geom(row_map=rm), out=torch.zeros_like(wide[0]), fidelity=mapped, **kw)
    assert torch.equal(out_w[:, :, rm.long()], out)
    assert torch.equal(spy.calls[-1][2], rm[sample_rows(S, N, 0, dev()).long()])
    assert torch.equal(mapped[0].rows, plain[0].rows)
    for name in NAMES:
        assert torch.equal(getattr(mapped[0], name), getattr(plain[0], name)), name
