"""Host: the Eval processors' shared call body (vorta_amd/attention/_eval.py) picks the route source and the launch rung the
two processors picked when each held its own copy.  Every launcher is replaced by a recorder that writes a marker into `out`;
the expected sequences below are written out from those two methods: per call (callee, batch item, operands given,
repair_above, fidelity keywords present), and for every call whether `text_len` / `text_valid` were passed (Hunyuan) or not (Wan).
The rows for a batch of two are the ones that matter: only item 0 receives the measurement's operands, only item 0 is
verified, and item 1 is launched from the repaired routes with `repair_above=None`."""
import pytest
import torch

LATENT, TILE, WINDOW, GROUP = (8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)
H, N, D, T, TE = 4, 384, 8, 16, 11
BOUND = 0.25
MARK = {"repaired": 1.0, "tiers": 2.0, "routed": 3.0, "op": 4.0}
SOURCES = ("rule_tiers", "rule_tuple", "tier_dict", "tier_repairable", "head_routing", "none")
SINKS = ("none", "fidelity", "expert_fidelity", "repair_above")
F3 = ("fidelity", "fidelity_heads", "fidelity_rows")
F4 = ("expert_fidelity", "fidelity", "fidelity_heads", "fidelity_rows")
TIERS_ERROR = "expert_fidelity: the per-expert sink does not go with a launch by precision tiers"
REPAIR_ERROR = "expert_fidelity: the per-expert sink does not go with repair_above"
ROUTE, SCORES = ("route", 0), ("route_scores",)


def _two(callee, given, fid):
    """items 0 and 1 of one rung: (callee, item, operands given, repair_above, fidelity keywords); `given`: item 0 only"""
    return [(callee, 0, given, "-", fid), (callee, 1, False, "-", fid)]


def _repair(given):
    return [("repaired", 0, given, BOUND, ("rows",)), ("repaired", 1, False, None, ())]


# (source, sink) -> the calls of a Wan call with B = 2, in order; a string: the ValueError raised after them
EXPECTED = {
    ("rule_tiers", "none"): [ROUTE] + _two("tiers", True, ()),
    ("rule_tuple", "none"): [ROUTE] + _two("op", False, ()),
    ("tier_dict", "none"): _two("tiers", False, ()),
    ("tier_repairable", "none"): _two("tiers", False, ()),
    ("head_routing", "none"): _two("op", False, ()),
    ("none", "none"): [SCORES] + _two("op", False, ()),
    ("rule_tiers", "fidelity"): [ROUTE] + _two("tiers", True, F3),
    ("rule_tuple", "fidelity"): [ROUTE] + _two("routed", False, F4),
    ("tier_dict", "fidelity"): _two("tiers", False, F3),
    ("tier_repairable", "fidelity"): _two("tiers", False, F3),
    ("head_routing", "fidelity"): _two("routed", False, F4),
    ("none", "fidelity"): [SCORES] + _two("routed", False, F4),
    ("rule_tiers", "expert_fidelity"): [ROUTE, TIERS_ERROR],
    ("rule_tuple", "expert_fidelity"): [ROUTE] + _two("routed", False, F4),
    ("tier_dict", "expert_fidelity"): [TIERS_ERROR],
    ("tier_repairable", "expert_fidelity"): [TIERS_ERROR],
    ("head_routing", "expert_fidelity"): _two("routed", False, F4),
    ("none", "expert_fidelity"): [SCORES] + _two("routed", False, F4),
    ("rule_tiers", "repair_above"): [ROUTE] + _repair(True),
    ("rule_tuple", "repair_above"): [ROUTE] + _repair(False),
    ("tier_dict", "repair_above"): _repair(False),
    ("tier_repairable", "repair_above"): _repair(False),
    ("head_routing", "repair_above"): _repair(False),
    ("none", "repair_above"): [SCORES] + _repair(False),
}
# the rungs that take the RoutedGeometry object: every one but the operator, which takes the geometry's keywords
NEEDS_GEOMETRY = {key: any(c[0] in ("route", "repaired", "tiers", "routed") for c in calls) for key, calls in EXPECTED.items()}


class _Recorder:
    def __init__(self, monkeypatch):
        from vorta_amd import routed
        from vorta_amd.attention import _eval
        from vorta_amd.routed import HeadRouting, RepairRecord, RouteRule, TierRoutes
        self.calls, self.text, self.routes_seen, self.geometries = [], [], [], 0
        self.head = lambda: HeadRouting.from_device(torch.zeros((3, H), dtype=torch.int32), torch.tensor([H, 0, 0], dtype=torch.int32))
        self.tier_routes = TierRoutes({"i8pv": self.head(), "native": self.head()}, torch.zeros(H, dtype=torch.int32),
                                      torch.zeros(H, dtype=torch.int32), {"i8pv": "fid-i8pv", "native": "fid-native"},
                                      {"i8pv": "operands-i8pv"}, torch.zeros((2, 3, H), dtype=torch.int32),
                                      torch.zeros((2, 3), dtype=torch.int32))
        self.rule_routing, self.rule_ids = self.head(), torch.zeros(H, dtype=torch.int32)

        def launcher(callee):
            def fake(q, k, v, routes, geom, *, out, **kw):
                assert q.shape[0] == k.shape[0] == v.shape[0] == out.shape[0] == 1 and geom == "geometry"
                self.calls.append((callee, int(q[0, 0, 0, 0]), kw.get("operands") is not None, kw.get("repair_above", "-"),
                                   tuple(sorted(n for n in F4 + ("rows",) if n in kw))))
                self.text.append((kw.get("text_len", "absent"), kw.get("text_valid", "absent"), kw["model"]))
                self.routes_seen.append(routes)
                out.fill_(MARK[callee])
                if callee == "repaired":
                    rec = RepairRecord("pre-repair rows", None, None, None, None, "repaired routes")
                    return out, (rec if kw["repair_above"] is not None else None)
                return out
            return fake

        def operator(q, k, v, out, *, head_lists, head_counts, counts_host, latent, tile, window, group, rate, **kw):
            assert (tuple(latent), tuple(tile), tuple(window), tuple(group), rate) == (LATENT, TILE, WINDOW, GROUP, 0.5)
            self.calls.append(("op", int(q[0, 0, 0, 0]), False, "-", ()))
            self.text.append((kw.get("text_len", "absent"), kw.get("text_valid", "absent"), kw["model"]))
            self.routes_seen.append((head_lists, head_counts, counts_host))
            out.fill_(MARK["op"])

        def route(rule, q, k, v, geom, **kw):
            assert q.shape[0] == k.shape[0] == v.shape[0] == 1 and geom == "geometry"
            self.calls.append(("route", int(q[0, 0, 0, 0])))
            self.text.append((kw.get("text_len", "absent"), kw.get("text_valid", "absent"), kw["model"]))
            return self.tier_routes if rule.covers_precision else (self.rule_routing, self.rule_ids, "fid-of-the-rule")

        def route_scores(score, tau):
            assert tau == 0.3
            self.calls.append(("route_scores",))
            self.scored = (torch.zeros(H, dtype=torch.int32), torch.zeros((3, H), dtype=torch.int32), torch.tensor([H, 0, 0], dtype=torch.int32))
            return self.scored

        def geometry_for(**kw):
            self.geometries += 1
            return "geometry"

        monkeypatch.setattr(_eval, "routed_attention_repaired", launcher("repaired"))
        monkeypatch.setattr(_eval, "routed_attention_tiers", launcher("tiers"))
        # (looked up in vorta_amd.routed at every call: tests/test_hip_patch_routed_fidelity.py records the launches there)
        monkeypatch.setattr(routed, "routed_attention", launcher("routed"))
        monkeypatch.setattr(_eval, "geometry_for", geometry_for)
        monkeypatch.setattr(RouteRule, "route", route)
        monkeypatch.setattr(torch.ops.vorta, "route_scores", route_scores)
        monkeypatch.setattr(torch.ops.vorta, "routed_attention", operator)


def _drive(rec, source, sinks, model, B):
    """`resolve_routes` + `launch_routes` as the model's processor calls them; returns what the call was given and `out`"""
    from vorta_amd import torch_ops
    from vorta_amd.attention import _eval, get_group_info
    from vorta_amd.routed import RepairableRoutes, RouteRule
    text = dict(text_len=T, text_valid=TE) if model == "hunyuan" else {}
    rows = N + (T if model == "hunyuan" else 0)
    q, k, v = (torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1).expand(B, H, rows, D).contiguous() for _ in range(3))
    given = dict(head_routing=None, route_rule=None, tier_routing=None, route_sink=[])
    if source.startswith("rule"):
        given["route_rule"] = RouteRule("max_rel_error", 0.1, covers_precision=source == "rule_tiers")
    elif source == "tier_dict":
        given["tier_routing"] = {"i8pv": rec.head(), "native": rec.head()}
    elif source == "tier_repairable":
        given["tier_routing"] = RepairableRoutes(("i8pv", "native"), torch.zeros(H, dtype=torch.int32), torch.zeros(H, dtype=torch.int32),
                                                 torch.zeros((2, 3, H), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32))
    elif source == "head_routing":
        given["head_routing"] = rec.head()
    geometry = torch_ops.geometry_args(get_group_info(LATENT, GROUP, 0.5), WINDOW, TILE, LATENT)
    out = torch.zeros_like(q)
    routes = _eval.resolve_routes(q, k, v, geometry, model=model, routing_score=torch.full((B, H, 3), 1 / 3), tau_sparse=0.3,
                                  **given, **text)
    _eval.launch_routes(q, k, v, out, routes, geometry, model=model, fidelity_rows="rows", fidelity_heads="all", **sinks, **text)
    return given, out


def _sinks(sink):
    return {"none": {}, "fidelity": dict(fidelity=[]), "expert_fidelity": dict(expert_fidelity=[]),
            "repair_above": dict(repair_above=BOUND, repair_sink=[])}[sink]


@pytest.mark.parametrize("model,B", [("hunyuan", 1), ("wan", 1), ("wan", 2)])
@pytest.mark.parametrize("sink", SINKS)
@pytest.mark.parametrize("source", SOURCES)
def test_every_route_source_with_every_sink(source, sink, model, B, monkeypatch):
    rec = _Recorder(monkeypatch)
    want = [c for c in EXPECTED[source, sink] if isinstance(c, str) or len(c) < 3 or c[1] < B]
    error = want.pop() if isinstance(want[-1], str) else None
    sinks = _sinks(sink)
    if error is not None:
        with pytest.raises(ValueError, match=error):
            _drive(rec, source, sinks, model, B)
        assert rec.calls == want
        return
    given, out = _drive(rec, source, sinks, model, B)
    assert rec.calls == want
    assert rec.text == [((T, TE) if model == "hunyuan" else ("absent", "absent")) + (model,)] * len(rec.text)
    assert len(rec.text) == len([c for c in want if c != SCORES])
    launches = [c for c in want if len(c) > 2]
    assert [float(out[b].unique()) for b in range(B)] == [MARK[c[0]] for c in launches], "every item written by its own launch"
    assert rec.geometries == (1 if NEEDS_GEOMETRY[source, sink] else 0), "one geometry lookup, on the rungs that take the object"
    # what was launched: the rule's routes, the given tables (a RepairableRoutes by its views), or the scores' dispatch
    first = rec.routes_seen[0]
    if sink == "repair_above":
        assert first is {"rule_tiers": rec.tier_routes, "tier_dict": given["tier_routing"], "tier_repairable": given["tier_routing"],
                         "head_routing": given["head_routing"]}.get(source, first)
        if source == "rule_tuple":
            assert first[0] is rec.rule_routing and first[1] is rec.rule_ids
        if source == "none":
            assert first.lists is rec.scored[1] and first.counts_dev is rec.scored[2] and first.expert_ids is rec.scored[0]
        assert rec.routes_seen[1:] == ["repaired routes"] * (B - 1)
        assert len(sinks["repair_sink"]) == 1 and sinks["repair_sink"][0].fidelity == "pre-repair rows"
    elif launches[0][0] == "tiers":
        assert first is rec.tier_routes.routings if source == "rule_tiers" else isinstance(first, dict) and list(first) == ["i8pv", "native"]
    elif launches[0][0] == "routed":
        assert first is {"rule_tuple": rec.rule_routing, "head_routing": given["head_routing"]}.get(source, first)
    else:
        lists = {"rule_tuple": rec.rule_routing, "head_routing": given["head_routing"]}.get(source)
        assert first[0] is (rec.scored[1] if lists is None else lists.lists) and first[2] is None
    entries = given["route_sink"]
    if source == "rule_tiers":
        assert len(entries) == 1 and len(entries[0]) == 5 and entries[0][3] == "fid-native" and entries[0][4]["tiers"] == ("i8pv", "native")
    elif source == "rule_tuple":
        assert len(entries) == 1 and entries[0][0] is rec.rule_ids and entries[0][1] is rec.rule_routing.lists and entries[0][3] == "fid-of-the-rule"
    else:
        assert entries == []


def test_a_repair_files_the_rows_before_it_and_later_items_measure_themselves(monkeypatch):
    """`fidelity` beside `repair_above`: item 0's record is the repair's own, filed once; item 1 is launched with the sink"""
    rec = _Recorder(monkeypatch)
    sinks = dict(fidelity=[], repair_above=BOUND, repair_sink=[])
    _drive(rec, "head_routing", sinks, "wan", 2)
    assert rec.calls == [("repaired", 0, False, BOUND, ("rows",)), ("repaired", 1, False, None, F3)]
    assert sinks["fidelity"] == ["pre-repair rows"] and len(sinks["repair_sink"]) == 1


@pytest.mark.parametrize("source", SOURCES)
def test_expert_fidelity_does_not_go_with_a_repair(source, monkeypatch):
    rec = _Recorder(monkeypatch)
    with pytest.raises(ValueError, match=REPAIR_ERROR):
        _drive(rec, source, dict(expert_fidelity=[], repair_above=BOUND), "wan", 2)
    assert all(c[0] in ("route", "route_scores") for c in rec.calls)


def test_sequence_parallel_refusals_by_name():
    from vorta_amd.attention._eval import refuse_under_sequence_parallel
    refuse_under_sequence_parallel(None, None, None, None)
    for i, text in enumerate(("sampled_expert_fidelity: the per-expert measurement on sampled rows does not run under sequence "
                              r"parallelism \(its gather reads whole heads of one process\)",
                              "route_rule: routing by a measured error bound or FLOP budget does not run under sequence "
                              r"parallelism \(its gather reads whole heads of one process\)",
                              "tier_routing: launching by precision tiers does not run under sequence parallelism",
                              "repair_above: verifying and repairing launched routes does not run under sequence parallelism "
                              r"\(its dense repair launch reads whole heads of one process\)")):
        args = [None] * 4
        args[i] = 0.5
        with pytest.raises(NotImplementedError, match="^" + text + "$"):
            refuse_under_sequence_parallel(*args)
    with pytest.raises(NotImplementedError, match="^sampled_expert_fidelity"):  # (the first keyword given names the refusal)
        refuse_under_sequence_parallel([], object(), {}, 0.1)
