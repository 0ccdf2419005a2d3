"""GPU: the Eval processors' shared call body (vorta_amd/attention/_eval.py) launches what each processor launched when it held
its own copy.  The geometry of tests/test_hip_processors.py (384 video tokens, 6 heads, bf16); every comparison is for EQUALITY
with the direct `routed.routed_attention_tiers` / `routed.routed_attention_repaired` calls on the processor's own q, k, v: per
batch item, item 0 alone on the measurement's operands, item 0 alone verified, item 1 launched from the repaired routes."""
import pytest
import torch
from torch import nn

from _util import dev
from test_hip_processors import GROUP, H, LATENT, S, TILE, WINDOW, _HyFakeAttn

pytestmark = pytest.mark.gpu
N_ROWS, SEED, HIDDEN = 64, 3, 64


class _WanAttn(nn.Module):
    """projections into 6 heads of 128, no norm, no output projection: the call returns the attention output, heads merged"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(7)
        self.heads, self.add_k_proj, self.norm_q, self.norm_k = H, None, None, None
        self.to_q, self.to_k, self.to_v = (nn.Linear(HIDDEN, H * 128) for _ in range(3))
        self.to_out = nn.ModuleList([nn.Identity(), nn.Identity()])
        self.to(dev()).to(torch.bfloat16)


def _geometry_kw():
    from vorta_amd import torch_ops
    from vorta_amd.attention import get_group_info
    from vorta_amd.routed import geometry_for
    kw = dict(lowres_group_info=get_group_info(LATENT, GROUP, 0.5, dev()), window_size=WINDOW, tile_size=TILE, latent_shape=LATENT)
    return kw, geometry_for(**torch_ops.geometry_args(kw["lowres_group_info"], WINDOW, TILE, LATENT), device=dev())


def _device_routing(experts):
    from vorta_amd.routed import HeadRouting
    host = HeadRouting.from_expert_ids(experts, dev())
    return HeadRouting.from_device(host.lists, torch.tensor(host.counts_host, dtype=torch.int32).to(dev()))


def test_wan_batch_of_two_follows_item_zero_through_tiers_and_repair():
    import vorta_amd.routed as rt
    from vorta_amd.attention import WanAttnProcessorTripleEval
    attn, proc = _WanAttn(), WanAttnProcessorTripleEval(check_input=True)
    torch.manual_seed(11)
    hidden = torch.randn((2, S, HIDDEN), device=dev()).to(torch.bfloat16)  # two distinct items
    score = torch.full((2, H, 3), 1.0 / 3, device=dev())
    kw, geom = _geometry_kw()
    rows = rt.sample_rows(S, N_ROWS, SEED, dev())
    call = lambda **more: proc(attn, hidden, None, None, None, tau_sparse=0.3, routing_score=score, **kw, **more)  # noqa: E731
    before = rt.DEFAULT_FP8
    try:
        with torch.no_grad():
            q, k, v, _ = proc._input_proj(attn, hidden, None, None)
            # (a) tier routes measured on item 0, launched as given: every item converts its own operands
            rt.set_attention_precision("auto8")
            routes = rt.route_by_fidelity(q[:1], k[:1], v[:1], geom, model="wan", rows=rows, max_rel_error=0.1, tiers=rt.tiers_of())
            assert tuple(routes.routings) == ("i8pv", "fp8pv", "native")
            got = call(tier_routing=routes.routings)
            buf, out = proc._new_out(q)
            for b in range(2):
                rt.routed_attention_tiers(q[b:b + 1], k[b:b + 1], v[b:b + 1], routes.routings, geom, model="wan",
                                          out=out[b:b + 1], operands=None)
            assert torch.equal(got, buf.flatten(2, 3)) and not torch.equal(got[0], got[1])
            # (c) a rule that covers the precision: item 0 is launched on the operands its measurement prepared, item 1
            # converts its own -- with item 0's operands its rows would be attention over item 0's keys and values
            rule = rt.RouteRule("max_rel_error", 0.1, n_rows=N_ROWS, seed=SEED, covers_precision=True)
            entries = []
            got = call(route_rule=rule, route_sink=entries)
            measured = rule.route(q[:1], k[:1], v[:1], geom, model="wan")
            assert isinstance(measured, rt.TierRoutes) and set(measured.operands) == {"i8pv", "fp8pv"}
            buf, out = proc._new_out(q)
            for b in range(2):
                rt.routed_attention_tiers(q[b:b + 1], k[b:b + 1], v[b:b + 1], measured.routings, geom, model="wan",
                                          out=out[b:b + 1], operands=measured.operands if b == 0 else None)
            assert torch.equal(got, buf.flatten(2, 3)) and len(entries) == 1 and len(entries[0]) == 5
            assert torch.equal(entries[0][4]["tier_ids"], measured.tier_ids)
            # (b) a device routing verified against a bound of 0: every sparse head of item 0 is re-run dense and the tables
            # are rewritten; item 1 launches the rewritten tables
            rt.set_attention_precision("native")
            experts = [(1, 2, 0)[h % 3] for h in range(H)]
            routing, sink = _device_routing(experts), []
            got = call(head_routing=routing, repair_above=0.0, repair_sink=sink, fidelity_rows=rows)
            direct = _device_routing(experts)
            buf, out = proc._new_out(q)
            _, repaired = rt.routed_attention_repaired(q[:1], k[:1], v[:1], direct, geom, repair_above=0.0, rows=rows,
                                                       operands=None, model="wan", out=out[:1])
            rt.routed_attention_repaired(q[1:2], k[1:2], v[1:2], repaired.routes, geom, repair_above=None, model="wan", out=out[1:2])
            plain = call(head_routing=_device_routing(experts))
    finally:
        rt.DEFAULT_FP8 = before
    assert torch.equal(got, buf.flatten(2, 3)) and not torch.equal(got, plain)
    assert len(sink) == 1 and isinstance(sink[0], rt.RepairRecord)
    assert sink[0].state_of_head.tolist() == [0 if e == 0 else 2 for e in experts] == repaired.state_of_head.tolist()
    assert int(sink[0].repair_count) == sum(e != 0 for e in experts) >= 1
    for tables in (routing, direct):  # the tables after the call are the repaired ones
        assert tables.counts_dev.tolist() == [H, 0, 0] and tables.lists[0].tolist() == list(range(H))


def test_hunyuan_rule_repair_and_fidelity_in_one_call():
    import vorta_amd.routed as rt
    from vorta_amd.attention import HunyuanVideoFlashAttnProcessorTripleEval
    T, te = 16, 11
    attn, proc = _HyFakeAttn(HIDDEN, False, torch.bfloat16, seed=3), HunyuanVideoFlashAttnProcessorTripleEval(check_input=True)
    torch.manual_seed(5)
    hidden = torch.randn((1, S, HIDDEN), device=dev()).to(torch.bfloat16)
    enc = torch.randn((1, T, HIDDEN), device=dev()).to(torch.bfloat16)
    ang = torch.rand((S, 64), device=dev()) * 6.28
    rope = (ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1))
    mask = torch.zeros((1, 1, 1, S + T), dtype=torch.bool, device=dev())
    mask[..., :S + te] = True
    kw, geom = _geometry_kw()
    rows = rt.sample_rows(S, N_ROWS, SEED, dev())
    rule = rt.RouteRule("max_flops_share", 0.8, n_rows=N_ROWS, seed=SEED)
    fidelity, repairs, routed = [], [], []
    before = rt.DEFAULT_FP8
    try:
        rt.set_attention_precision("native")
        with torch.no_grad():
            got = proc(attn, hidden, enc, mask, rope, routing_score=torch.full((1, H, 3), 1.0 / 3, device=dev()), tau_sparse=0.3,
                       route_rule=rule, route_sink=routed, repair_above=0.0, repair_sink=repairs, fidelity=fidelity,
                       fidelity_rows=rows, **kw)
            q, k, v, _ = proc._project(attn, hidden, enc, rope)
            text = dict(model="hunyuan", text_len=T, text_valid=te)
            routing, ids, _ = rule.route(q, k, v, geom, **text)
            buf, out = proc._new_out(q)
            _, repaired = rt.routed_attention_repaired(q, k, v, (routing, ids), geom, repair_above=0.0, rows=rows, operands=None,
                                                       out=out, **text)
            want = proc._output(attn, buf, T)
    finally:
        rt.DEFAULT_FP8 = before
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert len(fidelity) == len(repairs) == len(routed) == 1 and fidelity[0] is repairs[0].fidelity
    assert repairs[0].state_of_head.tolist() == repaired.state_of_head.tolist() and int(repairs[0].repair_count) >= 1
    assert torch.equal(routed[0][0], ids) and len(routed[0]) == 4
