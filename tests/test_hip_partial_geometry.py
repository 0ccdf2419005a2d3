"""GPU: tile and coreset windows that do not divide the latent grid (DESIGN.md "Partial geometry"), against the float64
restatement of tests/_partial_geometry_restate.py: tables, the coreset lists, every expert and the soft mixture forward and
backward, the 8-bit precisions, device-side routing, and a dividing control that must not change by a bit."""
import math

import numpy as np
import pytest
import torch

import _partial_geometry_restate as R
from _util import check, dev

pytestmark = pytest.mark.gpu

WINDOW, GROUP = (3, 3, 3), (2, 2, 2)
# (latent, tile): two length classes with thin tiles in all three dimensions; three lengths from four (t, h) extent pairs and
# C = 90; one thin tile that spans a whole dimension; and four lengths, which with Hunyuan's text launch makes seven
# launches -- more than one fused grid takes; and a tile that does not divide under a coreset window that does (C = 0)
GEOMS = {"thin3": ((7, 5, 6), (2, 2, 4)), "four": ((7, 9, 6), (2, 2, 4)), "span": ((7, 5, 6), (8, 2, 4)),
         "seven": ((7, 7, 7), (2, 2, 2)), "tile_only": ((6, 4, 6), (4, 2, 4))}
CONTROL = ((8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2))
T_TEXT, T_VALID = 64, 40
H = 4
MODELS = ("wan", "hunyuan")


@pytest.fixture(autouse=True)
def partial_on():
    from vorta_amd import _partial
    before = _partial._partial_geometry
    _partial.set_partial_geometry(True)
    yield
    _partial._partial_geometry = before


def _text(model):
    return (T_TEXT, T_VALID) if model == "hunyuan" else (0, 0)


def _geom(name):
    from vorta_amd.routed import geometry_for
    latent, tile = GEOMS[name]
    return geometry_for(latent, tile, WINDOW, GROUP, 0.5, dev())


def _qkv(S, T, dtype, seed, heads=H):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return tuple(torch.randn((1, heads, S + T, 128), generator=gen).to(dtype).to(dev()) for _ in range(3))


def _visible(latent, tile, te):
    """(S, S + te) bool: the restatement's visibility of video and valid text keys for every video query"""
    S = latent[0] * latent[1] * latent[2]
    return np.concatenate([R.sta_visible(latent, tile, WINDOW), np.ones((S, te), dtype=bool)], axis=1)


# ------------------------------------------------------------------------------------------------------------- 1. tables
@pytest.mark.parametrize("name", list(GEOMS))
@pytest.mark.parametrize("mapped", [False, True])
def test_tables_against_the_restatement(name, mapped):
    from vorta_amd import ops
    latent, tile = GEOMS[name]
    S, te = latent[0] * latent[1] * latent[2], T_VALID
    rm = None
    if mapped:  # synthetic injective row map over video and text tokens
        rm = (torch.arange(S + T_TEXT) * 3 + 1).to(torch.int32).to(dev())
    q_rows, kv_rows, lens = ops.sta_build_tables_partial(latent, tile, WINDOW, te, dev(), row_map=rm)
    n_tiles, n_lists, stride, lens2 = ops.sta_partial_sizes(latent, tile, WINDOW, te)
    assert kv_rows.shape == (n_lists, stride) and lens == lens2 and max(lens) == stride
    to_tok = (lambda r: r) if rm is None else (lambda r: (r - 1) // 3)
    assert np.array_equal(to_tok(q_rows.cpu().numpy()), R.tile_major_order(latent, tile))
    vis = _visible(latent, tile, te)
    kv = to_tok(kv_rows.cpu().numpy())
    fc = R.window_first_count(latent, tile, WINDOW)
    nf = [int(f.max()) + 1 for f, _ in fc]
    t3 = R.coords(latent) // np.asarray(tile)
    lid = (fc[0][0][t3[:, 0]] * nf[1] + fc[1][0][t3[:, 1]]) * nf[2] + fc[2][0][t3[:, 2]]
    assert n_lists == nf[0] * nf[1] * nf[2] and set(lid.tolist()) == set(range(n_lists))
    member = np.zeros((n_lists, S + te), dtype=bool)
    for l in range(n_lists):
        rows = kv[l, :lens[l]]
        assert len(set(rows.tolist())) == lens[l], "the rows of one key list are distinct"
        member[l, rows] = True
    assert np.array_equal(member[lid], vis)  # as sets, for every query token
    assert sorted({n - te for n in lens}) == R.key_list_lengths(latent, tile, WINDOW)
    assert n_tiles == int(np.prod(R.n_tiles(latent, tile)))


# ------------------------------------------------------------------------------------------------------------ 2. coreset
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_coreset_lists_of_a_cropped_latent(dtype):
    """latent (7,4,4) with window (2,2,2): the crop is the first six frames, whose 96 tokens are contiguous -- the window part
    of the lists must be, bit for bit, what the dividing selection writes for latent (6,4,4) over the same tensor"""
    from vorta_amd import ops
    latent, small, n_tail = (7, 4, 4), (6, 4, 4), 24
    S = 7 * 4 * 4
    cs = R.Coreset(latent, GROUP)
    assert (cs.G, cs.C, cs.n_keep) == (12, 16, 3) and np.array_equal(cs.remainder, np.arange(96, 112))
    x = _qkv(S, n_tail, dtype, 3, heads=3)[0][0]
    keep, drop, kv = ops.coreset_select(x, latent, GROUP, cs.n_keep, tail_first=S, n_tail=n_tail, want_kv=True, partial=True)
    keep0, drop0, kv0 = ops.coreset_select(x, small, GROUP, cs.n_keep, want_kv=True)
    nw = cs.G * (1 + cs.n_keep)
    assert keep.shape == (3, cs.S_low + n_tail) and kv.shape == keep.shape and drop.shape == drop0.shape
    assert torch.equal(keep[:, :nw], keep0) and torch.equal(drop, drop0) and torch.equal(kv[:, :nw], kv0)
    rest = torch.cat([torch.arange(96, 112), S + torch.arange(n_tail)]).to(torch.int32).to(dev())
    assert torch.equal(keep[:, nw:], rest.expand(3, -1)) and torch.equal(kv[:, nw:], rest.expand(3, -1))
    # the layout of the restatement, for the kernel's own margin choice
    kept = keep[:, cs.G:nw].cpu().numpy().reshape(3, cs.G, cs.n_keep)
    for h in range(3):
        assert np.array_equal(keep[h].cpu().numpy(), cs.keep_layout(kept[h], n_tail))
    # device head count: slots past it are not written
    n_dev = torch.tensor([2], dtype=torch.int32, device=dev())
    a = ops.coreset_select(x, latent, GROUP, cs.n_keep, tail_first=S, n_tail=n_tail, partial=True, n_heads_dev=n_dev)[0]
    assert torch.equal(a[:2], keep[:2])
    with pytest.raises(ValueError):
        ops.coreset_select(x, (7, 1, 4), GROUP, cs.n_keep, partial=True)  # no whole window


def test_coreset_lists_of_a_latent_cropped_in_height_and_width():
    """latent (7,5,7) with window (2,2,2): the crop (6,4,6) changes the row and column strides.  The dividing selection over a
    contiguous COPY of the cropped box sees the same rows, so it ranks alike: its lists, mapped from the small grid's token ids
    to the large one's, must be the window part of the partial lists bit for bit"""
    from vorta_amd import ops
    latent, small, n_tail = (7, 5, 7), (6, 4, 6), 8
    S = 7 * 5 * 7
    cs = R.Coreset(latent, GROUP)
    assert (cs.G, cs.C) == (18, S - 144)
    x = _qkv(S, n_tail, torch.bfloat16, 6, heads=2)[0][0]
    big = torch.arange(S).view(latent)[:6, :4, :6].reshape(-1).to(dev())  # small-grid token -> large-grid token
    xs = x[:, big].contiguous()
    keep, drop, kv = ops.coreset_select(x, latent, GROUP, cs.n_keep, tail_first=S, n_tail=n_tail, want_kv=True, partial=True)
    keep0, drop0, kv0 = ops.coreset_select(xs, small, GROUP, cs.n_keep, want_kv=True)
    nw = cs.G * (1 + cs.n_keep)
    to_big = lambda t: big[t.long()].to(torch.int32)  # noqa: E731
    assert torch.equal(keep[:, :nw], to_big(keep0)) and torch.equal(drop, to_big(drop0)) and torch.equal(kv[:, :nw], to_big(kv0))
    rest = torch.cat([torch.as_tensor(cs.remainder), S + torch.arange(n_tail)]).to(torch.int32).to(dev())
    assert torch.equal(keep[:, nw:], rest.expand(2, -1)) and torch.equal(kv[:, nw:], rest.expand(2, -1))


def test_coreset_partial_entry_point_on_a_dividing_window_gives_the_old_lists():
    """the tile does not divide, the coreset window does: C = 0, the second kernel writes only the tail"""
    from vorta_amd import ops
    latent, n_tail = GEOMS["tile_only"][0], 24
    S = latent[0] * latent[1] * latent[2]
    geom = _geom("tile_only")
    assert geom.is_partial and geom.C == 0 and geom.S_low == geom.G * (1 + geom.n_keep)
    x = _qkv(S, n_tail, torch.float16, 7, heads=3)[0][0]
    kw = dict(tail_first=S, n_tail=n_tail, want_kv=True)
    for a, b in zip(ops.coreset_select(x, latent, GROUP, geom.n_keep, partial=True, **kw),
                    ops.coreset_select(x, latent, GROUP, geom.n_keep, **kw)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 3. forward, all experts
def _recorded(q, k, v, geom, model, **kw):
    """the three expert buffers of all heads and the launches as launched"""
    from vorta_amd.routed import HeadRouting, routed_attention
    t, te = _text(model)
    bufs, launches = [torch.empty_like(q) for _ in range(3)], []
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(q.shape[1], q.device), geom, model=model, text_len=t,
                     text_valid=te, expert_outs=bufs, fp8=False, record=launches, **kw)
    return bufs, launches


def _kernel_choice(launches, cs, te):
    """kept margins (H, G, n_keep) of the query side and the key rows (H, n_kv) of the coreset launch, checked against the layout"""
    low = next(c for c in launches if c.get("dup_rows") is not None)
    keep, drop, kvr = low["q_rows"].cpu().numpy(), low["dup_rows"].cpu().numpy(), low["kv_rows"].cpu().numpy()
    nw = cs.G * (1 + cs.n_keep)
    assert low["n_q"] == keep.shape[1] and low["q_valid"] == cs.S_low + te
    assert low["n_kv"] == cs.S_low + te and low["n_dup_pos"] == cs.G
    kept_q = keep[:, cs.G:nw].reshape(-1, cs.G, cs.n_keep)
    kept_k = []
    for h in range(keep.shape[0]):
        assert np.array_equal(keep[h], cs.keep_layout(kept_q[h], keep.shape[1] - cs.S_low))
        for w in range(cs.G):  # kept + dropped = the window's margins
            assert sorted(kept_q[h, w].tolist() + drop[h, w].tolist()) == sorted(cs.margins[w].tolist())
        keys = kvr[h, :cs.S_low + te]
        assert len(set(keys.tolist())) == keys.size
        km = np.asarray([t for t in keys if t < cs.S and cs.role[t] == 1])
        assert km.size == cs.G * cs.n_keep and all((cs.window[km] == w).sum() == cs.n_keep for w in range(cs.G))
        assert set(keys.tolist()) == set(cs.centres.tolist()) | set(cs.remainder.tolist()) | set(km.tolist()) | \
            set(range(cs.S, cs.S + te))
        kept_k.append(km)
    return kept_q, kept_k


def _check_sliding_launches(launches, latent, tile, te):
    """the sliding launches hold every query token once, and every block of a launch reads its tokens' visible set"""
    S = latent[0] * latent[1] * latent[2]
    vis = _visible(latent, tile, te)
    seen = np.zeros(S, dtype=int)
    sl = [c for c in launches if c["tag"] == "sliding"]
    for c in sl:
        qr, kvr = c["q_rows"].cpu().numpy(), c["kv_rows"].cpu().numpy()
        covered = np.zeros(c["n_q"], dtype=int)
        for g, a, b in c["q_block_table"].cpu().tolist():
            assert 0 < b - a <= c["block_rows"] and g < c["n_key_lists"]
            covered[a:b] += 1
            keys = kvr.reshape(-1)[g * c["kv_rows_stride_g"]: g * c["kv_rows_stride_g"] + c["n_kv"]]
            assert len(set(keys.tolist())) == c["n_kv"], "the first n_kv rows of a recorded key list are distinct"
            want = np.zeros(S + te, dtype=bool)
            want[keys] = True
            assert (vis[qr[a:b]] == want).all()
        assert (covered == 1).all()
        seen[qr[:c["n_q"]]] += 1
    assert (seen == 1).all()
    assert sorted(c["n_kv"] - te for c in sl) == R.key_list_lengths(latent, tile, WINDOW)
    return len(sl)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_forward_every_expert_mixed_routing_and_soft_mixture(name, model):
    from vorta_amd import ops
    from vorta_amd.routed import HeadRouting, routed_attention, soft_mixture_attention
    latent, tile = GEOMS[name]
    dtype = torch.bfloat16 if name in ("thin3", "seven", "tile_only") else torch.float16
    S = latent[0] * latent[1] * latent[2]
    t, te = _text(model)
    geom = _geom(name)
    assert geom.is_partial
    cs = R.Coreset(latent, GROUP)
    q, k, v = _qkv(S, t, dtype, 11)
    bufs, launches = _recorded(q, k, v, geom, model)
    n_sl = _check_sliding_launches(launches, latent, tile, te)
    assert len(launches) == 2 + n_sl + (1 if t else 0)
    if name == "seven" and model == "hunyuan":
        assert len(launches) > ops.MAX_FUSED  # goes out as two fused grids
    kept_q, kept_k = _kernel_choice(launches, cs, te)
    specs = R.expert_specs(latent, tile, WINDOW, cs, kept_q, kept_k, t, te)
    f64 = lambda x: x[0].double().cpu().numpy()  # noqa: E731
    qn, kn, vn = f64(q), f64(k), f64(v)
    refs = [R.attend(qn, kn, vn, *specs[e]) for e in range(3)]
    kwm = dict(model=model, text_len=t, text_valid=te)
    for e in range(3):
        alone = routed_attention(q, k, v, HeadRouting.from_expert_ids([e] * H, dev()), geom, **kwm)
        assert torch.equal(alone, bufs[e])
        for h in range(H):  # every row of every head
            check(alone[0, h], refs[e][h], dtype)
    experts = [0, 1, 2, 1]
    route = HeadRouting.from_expert_ids(experts, dev())
    mixed = routed_attention(q, k, v, route, geom, **kwm)
    for h, e in enumerate(experts):
        check(mixed[0, h], refs[e][h], dtype)
    assert torch.equal(mixed, routed_attention(q, k, v, route, geom, fused=False, **kwm))
    assert torch.equal(mixed, routed_attention(q, k, v, route, geom, concurrent=True, **kwm))
    gen = torch.Generator(device="cpu").manual_seed(5)
    sc = torch.softmax(torch.randn((1, H, 3), generator=gen), dim=-1).to(dtype).to(dev())
    soft = soft_mixture_attention(q, k, v, sc, geom, **kwm)
    ref = R.mixture(qn, kn, vn, sc[0].double().cpu().numpy(), specs)
    for h in range(H):
        check(soft[0, h], ref[h], dtype)
    if t > te:
        assert not soft[0, :, S + te:].any() and not mixed[0, :, S + te:].any()


# ---------------------------------------------------------------------------------------------------- dividing control
@pytest.mark.parametrize("model", MODELS)
def test_dividing_geometry_is_unchanged_by_the_switch(model):
    from vorta_amd import _partial
    from vorta_amd.routed import geometry_for
    latent, tile, window, group = CONTROL
    S = latent[0] * latent[1] * latent[2]
    t, te = _text(model)
    q, k, v = _qkv(S, t, torch.bfloat16, 2)
    runs = []
    for on in (False, True):
        _partial.set_partial_geometry(on)
        geom = geometry_for(latent, tile, window, group, 0.5, dev())
        assert geom.partial is on and not geom.is_partial
        bufs, launches = _recorded(q, k, v, geom, model)
        runs.append((geom, bufs, launches))
    (g0, b0, l0), (g1, b1, l1) = runs
    assert g0 is not g1  # the cache is keyed on the flag
    assert all(torch.equal(a, b) for a, b in zip(b0, b1))
    assert len(l0) == len(l1)
    for c0, c1 in zip(l0, l1):
        assert c0.keys() == c1.keys()
        for key in c0:
            if key in ("q", "k", "v", "out"):
                continue
            a, b = c0[key], c1[key]
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, key
    for te_ in (0, te):
        for a, b in zip(g0.sta_launch_tables(te_, 256), g1.sta_launch_tables(te_, 256)):
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b


# ----------------------------------------------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["thin3", "four", "span"])
def test_soft_mixture_backward_three_algorithms(name, model):
    from test_hip_attention_bwd import _bound  # the rule of the attention-backward tests: e_hip <= 2 e_torch
    from vorta_amd.routed import ATTENTION_BACKWARDS, soft_mixture_attention, soft_mixture_attention_autograd
    latent, tile = GEOMS[name]
    dtype = torch.float16 if name == "four" else torch.bfloat16
    S = latent[0] * latent[1] * latent[2]
    t, te = _text(model)
    geom = _geom(name)
    cs = R.Coreset(latent, GROUP)
    q, k, v = _qkv(S, t, dtype, 21)
    gen = torch.Generator(device="cpu").manual_seed(22)
    G = torch.randn(q.shape, generator=gen).to(dtype).to(dev())
    sc = torch.softmax(torch.randn((1, H, 3), generator=gen), dim=-1).to(dtype).to(dev())
    bufs, launches = _recorded(q, k, v, geom, model)
    kept_q, kept_k = _kernel_choice(launches, cs, te)
    specs = R.expert_specs(latent, tile, WINDOW, cs, kept_q, kept_k, t, te)

    def reference(dt):
        leaves = [x[0].detach().to(dt).requires_grad_(True) for x in (q, k, v)]
        s = sc[0].detach().to(dt).requires_grad_(True)
        out = R.mixture_torch(*leaves, s, specs)
        return torch.autograd.grad(out, leaves + [s], G[0].to(dt))

    ref, t16 = reference(torch.float64), reference(dtype)
    kwm = dict(model=model, text_len=t, text_valid=te)
    plain = soft_mixture_attention(q, k, v, sc, geom, **kwm)
    for algorithm in ATTENTION_BACKWARDS:
        grads = []
        for _ in range(2 if algorithm == "deterministic" else 1):
            leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
            out = soft_mixture_attention_autograd(*leaves, geom, backward=algorithm, **kwm)
            assert torch.equal(out, plain)
            (out * G).sum().backward()
            grads.append([x.grad for x in leaves])
        for name_, got, a, b in zip(("dq", "dk", "dv", "dscores"), grads[0], t16, ref):
            _bound(name_, got[0], a, b, f"{name} {model} {algorithm}")
        if algorithm == "deterministic":
            assert all(torch.equal(a, b) for a, b in zip(*grads)), "two deterministic backward passes differ"
        if t > te:
            assert not any(g[:, :, S + te:].any() for g in grads[0][:3])


# --------------------------------------------------------------------------------------------------- 5. 8-bit precisions
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("precision", ["auto8", "i8pv", "fp8pv"])
def test_eight_bit_precisions_against_native_on_structured_inputs(precision, model):
    from _structured_inputs import structured_layer
    from vorta_amd.routed import HeadRouting, routed_attention
    latent, tile = GEOMS["four"]
    S = latent[0] * latent[1] * latent[2]
    t, te = _text(model)
    experts = [0, 1, 2, 2]
    gen = torch.Generator(device=dev()).manual_seed(123)
    q, k, v = structured_layer(latent, experts, tile, GROUP, 0.05, gen, dev())
    if t:
        q, k, v = (torch.cat([x, torch.randn((1, H, t, 128), generator=gen, device=dev())], dim=2) for x in (q, k, v))
    q, k, v = (x.to(torch.float16).contiguous() for x in (q, k, v))
    geom = _geom("four")
    route = HeadRouting.from_expert_ids(experts, dev())
    kwm = dict(model=model, text_len=t, text_valid=te)
    native = routed_attention(q, k, v, route, geom, fp8=False, **kwm).float()
    out = routed_attention(q, k, v, route, geom, fp8=precision, **kwm).float()
    assert torch.isfinite(out).all()
    for h in range(H):
        a, b = out[0, h, :S + te], native[0, h, :S + te]
        psnr = 10 * math.log10((b.max() - b.min()).item() ** 2 / max(((a - b) ** 2).mean().item(), 1e-30))
        print(f"{precision} {model} head {h} (expert {experts[h]}): {psnr:.2f} dB")
        assert psnr >= 40.0, (precision, model, h, psnr)
    assert not out[0, :, S + te:].any()


# ------------------------------------------------------------------------------------------------- 6. device-side routing
def test_device_side_routing_on_a_partial_geometry_is_sync_free_and_equal():
    from vorta_amd import ops
    from vorta_amd.routed import HeadRouting, routed_attention
    dtype = torch.bfloat16
    latent, tile = GEOMS["four"]
    S, T, te = latent[0] * latent[1] * latent[2], T_TEXT, T_VALID
    torch.manual_seed(11)
    Hh, E = 6, 64
    temb = torch.randn((1, E), device=dev()).to(dtype)
    w = (torch.randn((3 * Hh, E), device=dev()) * 0.5).to(dtype)
    b = torch.zeros(3 * Hh, device=dev()).to(dtype)
    q, k, v = (torch.randn((1, Hh, S + T, 128), device=dev()).to(dtype) for _ in range(3))
    geom = _geom("four")
    geom.prebuild(te)  # per-prompt tables: built once, outside the sync-checked region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
    try:
        scores, expert, lists, counts = ops.router_route(temb, w, b, Hh, 0.3)
        out_dev = routed_attention(q, k, v, HeadRouting.from_device(lists, counts), geom, model="hunyuan", text_len=T,
                                   text_valid=te)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out_host = routed_attention(q, k, v, HeadRouting.from_expert_ids(expert.cpu().tolist(), dev()), geom,
                                model="hunyuan", text_len=T, text_valid=te)
    assert torch.equal(out_dev, out_host)
    assert len(set(expert.cpu().tolist())) >= 2  # the draw exercises more than one expert


# ------------------------------------------------------------------------------ coreset lists under a row map (Ulysses layout)
def test_coreset_partial_lists_honour_a_row_map():
    from vorta_amd import ops
    latent, n_tail = (7, 4, 4), 8
    S = 7 * 4 * 4
    x = _qkv(S, n_tail, torch.bfloat16, 4, heads=2)[0][0]
    rm = (torch.arange(S + n_tail) * 2 + 1).to(torch.int32).to(dev())
    wide = torch.zeros((2, 2 * (S + n_tail) + 1, 128), dtype=x.dtype, device=dev())
    wide[:, rm.long()] = x  # token i lives in row rm[i]
    plain = ops.coreset_select(x, latent, GROUP, 3, tail_first=S, n_tail=n_tail, want_kv=True, partial=True)
    mapped = ops.coreset_select(wide, latent, GROUP, 3, tail_first=S, n_tail=n_tail, want_kv=True, partial=True, row_map=rm)
    for a, b in zip(plain, mapped):
        assert torch.equal(rm[a.long()], b)


# ------------------------------------------------------------------------------------- 7. processors and a patched mini model
P_LATENT, P_TILE, P_GROUP = (5, 6, 8), (2, 3, 4), (2, 3, 2)  # a thin last tile in time; the coreset crop leaves one frame: C = 48
P_T, P_TE = 16, 11


def _mini(family, dtype, train):
    import _mini_diffusers as M
    import vorta.patch.modeling_hunyuan as mh
    import vorta.patch.modeling_wan as mw
    mod = mh if family == "hunyuan" else mw
    torch.manual_seed(0)
    model = (M.MiniHunyuanTransformer if family == "hunyuan" else M.MiniWanTransformer)().to(dev()).to(dtype)
    if train:
        mod.apply_vorta_transformer(model, train_router=True, router_dtype=dtype, attn_processor_kwargs={"differentiable": True})
    else:
        mod.apply_vorta_transformer(model)
    g = torch.Generator().manual_seed(1)  # wide logits, layers that disagree (tests/test_hip_patch.py)
    for m in model.modules():
        if type(m).__name__ == "Router":
            m.linear.weight.data = (torch.randn(m.linear.weight.shape, generator=g) * 0.5).to(m.linear.weight)
            m.linear.bias.data = (torch.randn(m.linear.bias.shape, generator=g) * 2.0).to(m.linear.bias)
    return model


def _mini_kwargs(family, tau_sparse=None):
    """what a checkpoint's config.json hands over: a geometry that does not divide the latent grid"""
    from vorta.patch.utils import prepare_hunyuan_self_attn_kwargs, prepare_wan_self_attn_kwargs
    prepare = prepare_hunyuan_self_attn_kwargs if family == "hunyuan" else prepare_wan_self_attn_kwargs
    return prepare(dict(latent_shape=P_LATENT, window_size=WINDOW, tile_size=P_TILE, lowres_window_size=P_GROUP,
                        lowres_reduction_rate=0.5), dev(), tau_sparse=tau_sparse)


def _mini_inputs(family, dtype):
    g = torch.Generator(device=dev()).manual_seed(1)
    hidden = torch.randn((1, 4) + P_LATENT, device=dev(), generator=g).to(dtype)
    if family == "wan":
        return dict(hidden_states=hidden, timestep=torch.tensor([412.0], device=dev()),
                    encoder_hidden_states=torch.randn((1, 20, 24), device=dev(), generator=g).to(dtype))
    mask = torch.zeros((1, P_T), device=dev())
    mask[:, :P_TE] = 1
    return dict(hidden_states=hidden, timestep=torch.tensor([637.0], device=dev()),
                encoder_hidden_states=torch.randn((1, P_T, 24), device=dev(), generator=g).to(dtype),
                encoder_attention_mask=mask, pooled_projections=torch.randn((1, 16), device=dev(), generator=g).to(dtype),
                guidance=torch.tensor([6000.0], device=dev()).to(dtype))


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_patched_mini_model_runs_and_trains_a_router_step(family):
    import _patch_training_restate as PR
    from vorta.patch import routing_scores_of
    from vorta_amd import _partial, routed
    dtype = torch.bfloat16
    inp = _mini_inputs(family, dtype)
    _partial.set_partial_geometry(False)
    with pytest.raises(ValueError, match="does not divide latent shape"):
        _mini_kwargs(family)
    _partial.set_partial_geometry(True)
    kw = _mini_kwargs(family)
    assert routed.geometry_for(P_LATENT, P_TILE, WINDOW, P_GROUP, 0.5, dev()).C == 48
    # inference: the Eval processors behind torch.ops.vorta.routed_attention
    with torch.no_grad():
        out = _mini(family, dtype, train=False)(**inp, return_dict=False,
                                                self_attention_kwargs=_mini_kwargs(family, tau_sparse=0.3))[0]
    assert out.shape == inp["hidden_states"].shape and torch.isfinite(out.float()).all()
    # training: the Train processors with differentiable=True, one step on the routers
    previous = routed._attention_backward
    routed.set_attention_backward("deterministic")
    try:
        model = _mini(family, dtype, train=True)
        routers = PR.router_parameters(model)
        before = {n: p.detach().clone() for n, p in routers.items()}
        out = model(**inp, return_dict=False, self_attention_kwargs=dict(kw), return_routing_scores=True)
        cot = torch.randn(out[0].shape, generator=torch.Generator().manual_seed(17)).to(dtype).to(dev())
        loss = PR.training_loss(out[0], routing_scores_of(model), cot, torch.float32)
        loss.backward()
        for n, p in routers.items():
            assert p.grad is not None and torch.isfinite(p.grad.float()).all() and p.grad.any(), n
        with torch.no_grad():  # one SGD step, the rate per tensor large enough to show in 16-bit weights
            for p in routers.values():
                p -= (0.1 * p.abs().max() / p.grad.abs().max()).to(p.dtype) * p.grad
        assert all(not torch.equal(before[n], p.detach()) for n, p in routers.items())
    finally:
        routed._attention_backward = previous
