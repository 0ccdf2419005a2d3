"""The 16-bit fused grid in ticket order (vorta_attn_fwd_batch_tickets) against the static order of its block indices, and the
waves that skip the key loop because all their rows lie past q_valid.  Neither changes what a logical workgroup computes, so
every comparison here is on bits."""
import numpy as np
import pytest
import torch

from _util import dev

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, GROUP = (6, 8, 8), (3, 4, 4), (3, 3, 3), (3, 2, 2)
S = LATENT[0] * LATENT[1] * LATENT[2]
T, TE = 64, 40
H = 8
# heads per expert (8 heads, the last case 7): shares that do not divide by 8, an empty segment, fewer live workgroups than
# XCD classes
COUNTS = [(3, 3, 2), (1, 0, 7), (0, 8, 0), (5, 1, 1)]


def bits(x):
    return x.contiguous().view(torch.int16)


def experts_of(counts, seed=0):
    ids = np.array([0] * counts[0] + [1] * counts[1] + [2] * counts[2])
    return np.random.default_rng(seed).permutation(ids).tolist()


def qkv(dtype, seed, rows=S + T, heads=H, lead=(1,)):
    gen = torch.Generator(device=dev()).manual_seed(seed)
    return tuple(torch.randn(lead + (heads, rows, 128), generator=gen, device=dev(), dtype=dtype) for _ in range(3))


@pytest.fixture(scope="module")
def geom():
    from vorta_amd.routed import RoutedGeometry
    return RoutedGeometry(LATENT, TILE, WINDOW, GROUP, 0.5, dev())


def routing_of(counts, device_routes):
    from vorta_amd import ops
    from vorta_amd.routed import HeadRouting
    experts = experts_of(counts)
    if not device_routes:
        return HeadRouting.from_expert_ids(experts, dev())
    sc = torch.zeros((1, len(experts), 3), device=dev())
    for h, e in enumerate(experts):
        sc[0, h, e] = 1.0
    _, lists, cnt = ops.route_scores(sc, 0.3)
    return HeadRouting.from_device(lists, cnt)  # every launch sized for H slots: the slots past the count are dead


def run(q, k, v, routing, geom, tickets, monkeypatch, out=None):
    from vorta_amd import ops
    from vorta_amd.routed import routed_attention
    monkeypatch.setattr(ops, "FUSED_TICKETS", 1 if tickets else 0)
    if out is None:  # a NaN pattern: a row nobody writes shows
        out = torch.full_like(q, float("nan"))
    return routed_attention(q, k, v, routing, geom, model="hunyuan", text_len=T, text_valid=TE, out=out, fused=True, fp8=False)


def drawn(clear=False):
    """what the current stream's ticket counters hold: the draws of the last grid in ticket order there (each launch zeroes
    them first), 0 where none has run; clear=True zeroes them, so that a later non-zero reading is a later grid's"""
    from vorta_amd import ops
    ws = ops._ticket_ws.get((dev().index, ops._stream()))
    if ws is None:
        return 0
    if clear:
        ws.zero_()
    return int(ws.sum().item())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("device_routes", [False, True])
@pytest.mark.parametrize("counts", COUNTS)
def test_ticket_order_equals_static_order(counts, device_routes, dtype, geom, monkeypatch):
    q, k, v = qkv(dtype, 5, heads=sum(counts))
    routing = routing_of(counts, device_routes)
    ref = run(q, k, v, routing, geom, False, monkeypatch)
    drawn(clear=True)
    out = run(q, k, v, routing, geom, True, monkeypatch)
    if device_routes or sum(c > 0 for c in counts) > 1:  # (one live expert on the host is one plain launch: no fused grid)
        assert drawn() > 0  # the counters advanced: the grid did take tickets
    assert torch.equal(bits(out), bits(ref))
    assert not torch.isnan(out[0, :, :S + TE].float()).any()  # every valid row written
    assert torch.all(bits(out[0, :, S + TE:]) == 0)


def test_ticket_order_is_deterministic_and_resets(geom, monkeypatch):
    q, k, v = qkv(torch.float16, 6)
    r0, r1 = routing_of((3, 3, 2), False), routing_of((1, 0, 7), True)
    ref0, ref1 = (run(q, k, v, r, geom, False, monkeypatch) for r in (r0, r1))
    outs = [run(q, k, v, r0, geom, True, monkeypatch) for _ in range(20)]  # one stream, one workspace, no sync between
    for o in outs:
        assert torch.equal(bits(o), bits(ref0))
    # another routing straight after through the same counters, and back: each launch starts from zero
    a = run(q, k, v, r1, geom, True, monkeypatch)
    b = run(q, k, v, r0, geom, True, monkeypatch)
    assert torch.equal(bits(a), bits(ref1)) and torch.equal(bits(b), bits(ref0))


def test_ticket_order_under_graph_replay(geom, monkeypatch):
    from vorta_amd import ops
    dtype = torch.float16
    routing = routing_of((3, 3, 2), False)
    q, k, v = qkv(dtype, 7)
    out = torch.full_like(q, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(q, k, v, routing, geom, True, monkeypatch, out=out)  # warm-up: the stream's counters exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.graph(graph, stream=side):
            run(q, k, v, routing, geom, True, monkeypatch, out=out)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for seed in (8, 9, 10):
        for dst, src in zip((q, k, v), qkv(dtype, seed)):
            dst.copy_(src)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        ref = run(q, k, v, routing, geom, False, monkeypatch)
        assert torch.equal(bits(got), bits(ref)), seed


def test_more_than_one_round_of_workgroups(monkeypatch):
    """two dense segments of 8 heads x 141 query blocks = 2 256 workgroups, two key blocks each; the second one ends in rows
    past q_valid (a workgroup that is all past it, and one cut in the middle of a wave)"""
    from vorta_amd import ops
    dtype = torch.float16
    n_q, n_kv = 141 * 256, 128
    gen = torch.Generator(device=dev()).manual_seed(11)
    qs = [torch.randn((H, n_q, 128), generator=gen, device=dev(), dtype=dtype) for _ in range(2)]
    k, v = (torch.randn((H, n_kv, 128), generator=gen, device=dev(), dtype=dtype) for _ in range(2))
    valid = [n_q, n_q - 300]

    def launch(tickets, q_valid):
        monkeypatch.setattr(ops, "FUSED_TICKETS", 1 if tickets else 0)
        outs = [torch.full_like(q, float("nan")) for q in qs]
        ops.attn_fwd_batch([dict(q=q, k=k, v=v, out=o, n_q=n_q, n_kv=n_kv, q_valid=qv, block_rows=256)
                            for q, o, qv in zip(qs, outs, q_valid)])
        return outs

    plan = [ops._plan(ops._attn_args(q, k, v, q, n_q=n_q, n_kv=n_kv, block_rows=256)[0]) for q in qs]
    assert sum(nwg for _, nwg, _ in plan) > 2048
    whole = launch(False, [n_q, n_q])  # every row computed, static order
    ref = launch(False, valid)
    drawn(clear=True)
    out = launch(True, valid)
    # the drawing itself: the fetch-and-add hands out every value once, so a counter that reached its share has handed out
    # each logical workgroup of that share exactly once; what it holds beyond the share are draws that came too late
    cnt = ops._ticket_ws[(dev().index, ops._stream())].cpu().tolist()
    for s_, (_, nwg, _) in enumerate(plan):
        for x in range(8):
            share = nwg // 8 + (1 if x < nwg % 8 else 0)
            assert share <= cnt[s_ * 8 + x] <= share + 8 * 32, (s_, x, cnt[s_ * 8 + x], share)  # (late draws: a few per CU of a class at most)
    assert not any(cnt[8 * len(plan):])  # no other counter was touched
    print("draws beyond the shares:", sum(cnt) - sum(nwg for _, nwg, _ in plan))
    for o, r, w, qv in zip(out, ref, whole, valid):
        assert torch.equal(bits(o), bits(r))
        assert not torch.isnan(o.float()).any()  # every row written
        assert torch.equal(bits(o[:, :qv]), bits(w[:, :qv]))
        assert torch.all(bits(o[:, qv:]) == 0)


# ---- waves past q_valid skip the key loop ----
N_Q, N_KV = 512, 320  # two 256-row workgroups, five key blocks (the last one whole: 3 splits of 2 + 2 + 1)


@pytest.fixture(scope="module")
def past_inputs():
    gen = torch.Generator(device=dev()).manual_seed(12)
    rows = N_Q + 128  # the duplicates of the first 64 positions live behind the query rows
    q = torch.randn((2, rows, 128), generator=gen, device=dev(), dtype=torch.float16)
    k, v = (torch.randn((2, N_KV, 128), generator=gen, device=dev(), dtype=torch.float16) for _ in range(2))
    k_nan = k.clone()
    k_nan[:, 200] = float("nan")
    q_rows = torch.randperm(N_Q, generator=gen, device=dev()).to(torch.int32)
    kv_rows = torch.randperm(N_KV, generator=gen, device=dev()).to(torch.int32)
    dup_rows = (N_Q + torch.arange(128, device=dev(), dtype=torch.int32)).view(64, 2).contiguous()
    return dict(q=q, k=k, k_nan=k_nan, v=v, q_rows=q_rows, kv_rows=kv_rows, dup_rows=dup_rows)


MODES = {
    "dense": lambda d: dict(),
    "tables": lambda d: dict(q_rows=d["q_rows"], kv_rows=d["kv_rows"], dup_rows=d["dup_rows"], n_dup_pos=64),
    "splits": lambda d: dict(n_splits=3),
}


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("q_valid", [300, 320, 256], ids=["mid_wave", "wave_boundary", "workgroup_boundary"])
def test_rows_past_q_valid(q_valid, mode, variant, past_inputs):
    from vorta_amd import ops
    d = past_inputs
    kw = dict(MODES[mode](d), n_q=N_Q, n_kv=N_KV, block_rows=256, variant=variant)
    pos_row = d["q_rows"].long() if mode == "tables" else torch.arange(N_Q, device=dev())

    def launch(k, qv):
        out = torch.full_like(d["q"], float("nan"))
        ops.attn_fwd(d["q"], k, d["v"], out, q_valid=qv, **kw)
        return out

    for k in (d["k"], d["k_nan"]):
        whole = launch(k, N_Q)  # every position computed: what a position below q_valid must hold, bit for bit
        out = launch(k, q_valid)
        below, past = pos_row[:q_valid], pos_row[q_valid:]
        assert torch.equal(bits(out[:, below]), bits(whole[:, below]))
        assert torch.all(bits(out[:, past]) == 0)  # zero bits, with a NaN key row too: the position alone decides
        if mode == "tables":  # the duplicates of positions 0 ... 63 (all below q_valid) follow their source rows
            assert torch.equal(bits(out[:, N_Q:]), bits(whole[:, N_Q:]))
            assert torch.equal(bits(out[:, N_Q:].view(2, 64, 2, 128)[:, :, 0]), bits(out[:, pos_row[:64]]))
    assert not torch.isnan(launch(d["k"], q_valid)[:, pos_row].float()).any()
