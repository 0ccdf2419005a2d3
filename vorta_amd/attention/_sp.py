"""Sequence-parallel branch of the processors: zero-copy Ulysses (vorta_amd/ulysses/engine.py).

Replaces the per-expert all_to_all_4D / shrink_dim / all_gather choreography of the reference
(hunyuan.py:147-164,184-187,423-431,453-455,481-489,500-503; wan.py:110-117,138-139,146-147,245-248,267-268,
280-283,291-292): ALL heads are resharded once per layer, before routing, with one all_to_all_single per tensor whose
chunks are contiguous on both sides; routing then happens on the local heads, so any expert mix works under SP (the reference needs
h_e % P == 0 for every expert).
"""
from typing import Optional

import torch

from .. import ops
from .._partial import coreset_numbers, divides, partial_geometry, sliding_video_pairs
from ..routed import HeadRouting, geometry_for, precision_of, routed_attention
from ..ulysses import SP_STATE
from ..ulysses.state import PLACEMENTS, default_sp_groups, resolve_placement  # noqa: F401  (one rule for the processors and bench.py)
from ..ulysses.engine import (RecvOperands, UlyssesLayout, auto_kv_splits, balanced_head_order, balanced_placement, exchange_and_attend,
                              split_align, split_placement, slot_groups)

_LAYOUTS = {}
_BUFFERS = {}  # receive buffers per (geometry, head-slot count): kept when the layout cache is trimmed, least recently used out
# how many buffer sets stay resident: VORTA_SP_BUFFER_SETS, or (default) enough for every slot count one geometry can see --
# under 'uneven' / 'split' placement a rank holds between 1 and 2 H / P (+ 1) head slots from layer to layer, and a bound below
# that makes every layer a miss: 4 receive buffers reallocated and zero-filled per layer
MAX_BUFFER_SETS = int(__import__("os").environ.get("VORTA_SP_BUFFER_SETS", "0"))


def _buffer_set_limit(H: int, P: int) -> int:
    return max(2, MAX_BUFFER_SETS) if MAX_BUFFER_SETS > 0 else max(4, 2 * (H // max(P, 1)) + 2)
_ROUTINGS = {}  # (local expert ids, device) -> HeadRouting: the device tables are built once per distinct local mix
# slot groups: a number (default 1: exchange, then attend), or "auto" = `default_sp_groups` of the heads per rank and the
# precision (ulysses/state.py) -- ranked on an emulated wire only, so opt-in until a node run has measured the links
SP_GROUPS = __import__("os").environ.get("VORTA_SP_GROUPS", "1")
SP_GROUPS = SP_GROUPS if SP_GROUPS == "auto" else max(1, int(SP_GROUPS))


def _sp_groups(H: int, P: int) -> int:
    if SP_GROUPS != "auto":
        return int(SP_GROUPS)
    return default_sp_groups(H // max(P, 1), precision_of(None))
# e4m3 attention under sequence parallelism: v crosses the links as e4m3 (ulysses/engine.py VWire); VORTA_DEBUG=sp_v_wire=0 keeps
# the 16-bit exchange with the receive-side conversion (A/B; same bytes in the operand buffers either way)
SP_V_WIRE = __import__("vorta_amd._debug", fromlist=["flag"]).flag("sp_v_wire", "1") != "0"
# head placement (VORTA_SP_PLACEMENT; bench.py --placement follows the same rule through `resolve_placement`):
#   "auto" (default) = "even" when P divides the heads, "uneven" otherwise: the exchange with equal splits is the one every
#       test and rehearsal exercises most, and on balanced routes the two are the same placement;
#   "even"   = H/P heads on every rank, LPT order inside (ulysses/engine.py balanced_head_order);
#   "uneven" = the ranks' head COUNTS follow the layer's routes (balanced_placement: whole heads are a coarse unit when H/P is
#       small and the mix is skewed -- 24 heads with 4 full-attention ones on 8 ranks: heaviest rank 1.33 of the mean cost with
#       3 heads each, 1.02 with 1 + ... + 5); variable-split all_to_all_single, padded text all-gather;
#   "split"  = uneven, then full-attention heads give a range of their queries to the lightest ranks until the heaviest is
#       within 1 % of the mean (`split_placement`).  Opt-in, like the key splits below.
SP_PLACEMENT = __import__("os").environ.get("VORTA_SP_PLACEMENT", "auto")
# key splits of the full-attention / coreset launches: "1" (default), a number, or "auto" = per layer from this rank's count
# of workgroups (a rank whose one or two heads leave the chip under one round of workgroups: small models on many ranks;
# changes the summation order -- ulysses/engine.py, bench.py --kv-splits)
SP_KV_SPLITS = __import__("os").environ.get("VORTA_SP_KV_SPLITS", "1")


def _layout_only(H, S, T, D, device, dtype, counts=None, extra_slots=0) -> UlyssesLayout:
    """the layout of a head placement (cached: a few integers and a shared row map), without receive buffers"""
    rank, P = SP_STATE.group_local_rank, SP_STATE.sp_size
    counts = tuple(counts) if counts is not None else (H // P,) * P
    lkey = (H, S, T, D, P, rank, str(device), dtype, counts)
    if lkey not in _LAYOUTS:
        if len(_LAYOUTS) > 512:
            _LAYOUTS.clear()
        _LAYOUTS[lkey] = UlyssesLayout(H, S, T, D, P, rank, device, dtype, SP_STATE.group, counts=counts, extra_slots=extra_slots)
    return _LAYOUTS[lkey]


def _layout(H, S, T, D, device, dtype, counts=None, extra_slots=0):
    """(layout of this layer's head placement, receive buffers of this rank's head-slot count)"""
    rank, P = SP_STATE.group_local_rank, SP_STATE.sp_size
    lay = _layout_only(H, S, T, D, device, dtype, counts, extra_slots)
    # one buffer set per distinct slot count (at most 2 H / P of them); layouts -- one per distinct tuple of head counts, cheap:
    # a few integers and a shared row map -- are evicted on their own, so trimming them never drops gigabytes mid-run
    bkey = (H, S, T, D, P, rank, str(device), dtype, lay.Hl)
    if bkey not in _BUFFERS:
        # bounded: a set is 4 buffers of rows_total x D plus the 8-bit copies -- hundreds of MB to GB; a process that
        # sees several resolutions or text lengths keeps the `_buffer_set_limit` most recently used sets (every slot count of one geometry fits)
        while len(_BUFFERS) >= _buffer_set_limit(H, P):
            _BUFFERS.pop(next(iter(_BUFFERS)))
        _BUFFERS[bkey] = RecvOperands(lay)
    else:
        _BUFFERS[bkey] = _BUFFERS.pop(bkey)  # most recently used last
    return lay, _BUFFERS[bkey]


def _routing(local_experts: tuple, device, q_ranges: tuple = ()) -> HeadRouting:
    """HeadRouting.from_expert_ids builds a CPU tensor and copies it to the device (a host stall per layer on the
    sequence-parallel path): cached per distinct local expert tuple (at most 3^(H/P) of them, a handful in practice).
    `q_ranges`: ((slot, t0, t1), ...) for full-attention heads that compute a range of their queries here (placement 'split')"""
    key = (local_experts, str(device), q_ranges)
    r = _ROUTINGS.get(key)
    if r is None:
        if len(_ROUTINGS) > 4096:
            _ROUTINGS.clear()
        r = _ROUTINGS[key] = HeadRouting.from_expert_ids(list(local_experts), device,
                                                         q_ranges={i: (t0, t1) for i, t0, t1 in q_ranges} or None)
    return r


def place_heads(experts, cost, P: int, S: int, dense_only: bool = False, placement: Optional[str] = None, groups: Optional[int] = None):
    """(placement taken, head order, heads per rank, query ranges or None) of one layer: VORTA_SP_PLACEMENT (default `auto`)
    resolved by `resolve_placement`, then the engine's placement of that name.
    VORTA_SP_GROUPS (default 1; `auto` = `default_sp_groups`, chosen on an emulated wire): the local heads travel in that many
    slot groups (as equal as the slot count allows), so the exchange of one group overlaps the attention of another."""
    H = len(experts)
    groups = _sp_groups(H, P) if groups is None else groups
    placement = resolve_placement(SP_PLACEMENT if placement is None else placement, H, P)
    parts = None
    if placement == "split" and H >= P and not dense_only:
        # below whole heads: full-attention heads give a range of their queries to the lightest ranks (ulysses/engine.py
        # split_placement; the part that ends at the last video token keeps the head's text queries)
        order, counts, parts = split_placement(experts, cost, P, S, groups, align=split_align(S))
        if not any(x is not None for x in parts):
            parts = None
    elif placement in ("uneven", "split") and H >= P:
        order, counts = balanced_placement(experts, cost, P, groups)
    else:
        order, counts = balanced_head_order(experts, cost, P, min(groups, H // P)), [H // P] * P
    return placement, order, counts, parts


def sp_attention(q, k, v, T: int, routing_score: Optional[torch.Tensor], tau_sparse: Optional[float], *, model: str,
                 text_valid: int = 0, attention_mask=None, lowres_group_info=None, window_size=(3, 3, 3),
                 tile_size=(6, 8, 8), latent_shape=None, experts_host=None, fidelity: Optional[list] = None,
                 fidelity_rows=None, fidelity_heads: str = "sparse") -> torch.Tensor:
    """q,k,v: (1, H, S/P + T, D) local sequence shard with the replicated text at the end.
    Returns the attention output as a (1, S/P + T, H, D) buffer (text rows: all heads, gathered).
    fidelity: a list that receives one `ops.SampledFidelity` over all H heads with the GLOBAL head ids: every slot group's
    `routed_attention` call measures its local heads through the receive layout (the sampled rows composed with the group's
    row map), and the heads other ranks hold stay NaN with expert -1 (`gather_routed_fidelity` joins the ranks); heads under
    the `split` placement are never measured.  The dense reference needs the 16-bit v on this rank: precisions whose v
    crosses the links as e4m3 are refused.  None: the launches of today."""
    B, H, N, D = q.shape
    assert B == 1
    P = SP_STATE.sp_size
    Sl = N - T
    S = Sl * P
    if routing_score is None:  # dense for every head
        experts = [0] * H
        te = T
        if attention_mask is not None:  # host read, as hunyuan.py:169; the mask covers the global video (reference's
            # patched forward, modeling_hunyuan.py:86-88) or the local shard (stock diffusers forward)
            from .hunyuan import _valid_keys
            te = int(_valid_keys(attention_mask).item()) - (attention_mask.shape[-1] - T)
    elif experts_host is not None:  # dispatched by the step's route plan: no device read in this layer
        experts = list(experts_host)
        te = text_valid
    else:
        # balanced placement needs the routes on the host: one small read per layer (the reference reads
        # torch.nonzero per expert, hunyuan.py:633); routes depend only on the timestep
        experts = ops.route_scores(routing_score, tau_sparse)[0].cpu().tolist()
        te = text_valid
    dense_only = lowres_group_info is None
    # the precision switch (set_attention_precision / VORTA_ATTENTION_PRECISION) is about the ROUTED operator; dense
    # attention -- --native_attention, the PSNR reference -- stays in the dtype of q,k,v on one GPU and under SP alike
    precision = precision_of(None) if not dense_only else "native"
    if fidelity is not None and (dense_only or precision != "native"):
        # (refused here, before the placement, the layout and the exchange: nothing is allocated, sent or launched)
        raise ValueError("sp_attention(fidelity=...): " + ("a dense call has no routed output to measure" if dense_only else
                         f"under precision '{precision}' v crosses the links as e4m3 and the 16-bit dense reference cannot be "
                         "formed on this rank; measure the 8-bit precisions on one GPU"))
    if dense_only:
        cost = [1.0, 1.0, 1.0]
    else:  # expert costs from the geometry alone (the placement comes first: the layout follows from it)
        gw = tuple(int(x) for x in lowres_group_info.window_size)
        if partial_geometry() and not divides(latent_shape, tile_size, gw):
            # a partial geometry: S_low with its remainder tokens, and the true number of (query, key) pairs
            # of the sliding expert, whose key lists differ in length -- host integers, no table is built for them
            s_low = coreset_numbers(latent_shape, gw, lowres_group_info.reduction_rate)[3]
            cost = [float(S + te) ** 2, float(s_low + te) ** 2,
                    float(sliding_video_pairs(latent_shape, tile_size, window_size) + S * te)]
        else:
            g = gw[0] * gw[1] * gw[2]
            s_low = (S // g) * int(g * (1 - lowres_group_info.reduction_rate))
            _, _, n_kv = ops.sta_table_sizes(latent_shape, tile_size, window_size, te)
            cost = [float(S + te) ** 2, float(s_low + te) ** 2, float(S) * n_kv]
    placement, order, counts, parts = place_heads(experts, cost, P, S, dense_only)
    sp_attention.last_placement = placement  # (what a test or a curious caller reads back)
    lay, sb = _layout(H, S, T, D, q.device, q.dtype, counts, extra_slots=len(order) - H)
    groups = min(_sp_groups(H, P), min(counts))
    sg = slot_groups(lay.Hl, groups)
    sgs, _, _ = lay.grouping(len(sg))  # a slot group is a receive layout of its own inside the buffers (ulysses/engine.py)
    # the routed geometry composed with each group's row map (one per distinct slot count, cached)
    geoms = [None if dense_only else geometry_for(latent_shape, tile_size, window_size, lowres_group_info.window_size,
                                                  lowres_group_info.reduction_rate, q.device, row_map=g.lay.row_map) for g in sgs]
    shards = [x[0, :, :Sl] for x in (q, k, v)]
    texts = [x[0, :, Sl:] for x in (q, k, v)] if T else None
    me = SP_STATE.group_local_rank
    local = [experts[h] for h in order[lay.starts[me]:lay.starts[me + 1]]]
    local_parts = [None] * len(local) if parts is None else parts[lay.starts[me]:lay.starts[me + 1]]
    ranges_of = lambda g0, g1: tuple((i - g0,) + tuple(local_parts[i]) for i in range(g0, g1) if local_parts[i] is not None)
    kv_splits = 1
    if not dense_only and SP_KV_SPLITS != "1":
        kv_splits = auto_kv_splits(local, S, T, s_low) if SP_KV_SPLITS == "auto" else max(1, int(SP_KV_SPLITS))

    filed = {}  # slot group -> its routed_attention call's record (local head slots)
    if fidelity is not None and not torch.is_tensor(fidelity_rows):
        # the cached table is built here, on the current stream, before the slot groups fork onto theirs (as `prepare` builds)
        from ..routed import DEFAULT_FIDELITY_ROWS, sample_rows
        fidelity_rows = sample_rows(S, min(DEFAULT_FIDELITY_ROWS, S) if fidelity_rows is None else fidelity_rows, 0, q.device)
    vwire = sb.begin(lay, precision, SP_V_WIRE or precision != "fp8")  # (SP_V_WIRE: "fp8" only; the others always send e4m3 v)

    def attend(g0, g1, gi):
        qv, kv, vv, ov = (sgs[gi].head_view(b) for b in sb.bufs)
        if dense_only:
            rm = sgs[gi].lay.row_map
            ops.attn_fwd(qv, kv, vv, ov, n_q=S + T, n_kv=S + te, q_valid=S + te, q_rows=rm[:S + T], kv_rows=rm[:S + te])
        else:
            routed_attention(qv, kv, vv, _routing(tuple(local[g0:g1]), q.device, ranges_of(g0, g1)), geoms[gi],
                             model=model, text_len=T, text_valid=te, out=ov, operands=sb.operands(sgs[gi]),
                             kv_splits=kv_splits,
                             **({} if fidelity is None else dict(fidelity=filed.setdefault(gi, []), fidelity_rows=fidelity_rows,
                                                                 fidelity_heads=fidelity_heads)))

    def prepare():
        # everything `attend` caches is built here, on the current stream, before the slot groups fork onto theirs
        if not dense_only:
            for g in geoms:
                g.prebuild(te if model == "hunyuan" else 0)
            for g0, g1 in sg:
                _routing(tuple(local[g0:g1]), q.device, ranges_of(g0, g1))

    # the received heads are written straight into the (1, N, H, D) result the output projection reads
    buf = torch.empty((1, N, H, D), dtype=q.dtype, device=q.device)
    exchange_and_attend(lay, shards, sb.bufs, order, texts, sg, attend,
                        buf[0, :Sl].transpose(0, 1), buf[0, Sl:].transpose(0, 1) if T else None, vwire=vwire,
                        prepare=prepare, parts=parts)
    if fidelity is not None:
        mine = order[lay.starts[me]:lay.starts[me + 1]]
        fidelity.append(_global_routed_fidelity([(filed[gi][-1], mine[g0:g1]) for gi, (g0, g1) in enumerate(sg)], H))
    return buf


def _global_routed_fidelity(records, H: int) -> "ops.SampledFidelity":
    """the slot groups' records (local head slots; `heads`: their global ids) as one record over all H heads: NaN and expert
    -1 for the heads another rank holds"""
    first = records[0][0]
    dev = first.sq_ref.device
    nan = lambda: torch.full((H,), float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    out = ops.SampledFidelity(nan(), nan(), nan(), nan(), nan(), None, first.n, first.rows,
                              torch.full((H,), -1, dtype=torch.int32, device=dev))
    for rec, heads in records:
        idx = torch.tensor(list(heads), dtype=torch.long, device=dev)
        for name in ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref", "expert"):
            getattr(out, name).index_copy_(0, idx, getattr(rec, name))
    return out


def gather_routed_fidelity(fid: "ops.SampledFidelity") -> "ops.SampledFidelity":
    """this rank's statistics ((..., H) with the global head ids, NaN / expert -1 for heads it does not hold: `sp_attention`'s
    records, or a stack of them over layers) -> every rank's: one all-gather per tensor over the sequence-parallel group (a
    collective: every rank calls it), a head taken from the first rank that holds it.  A gloo group gathers host copies."""
    import torch.distributed as dist
    P = SP_STATE.sp_size
    staged = dist.get_backend(SP_STATE.group) == "gloo"

    def gather(t):
        src = t.cpu() if staged else t.contiguous()
        parts = [torch.empty_like(src) for _ in range(P)]
        dist.all_gather(parts, src, group=SP_STATE.group)
        return torch.stack(parts).to(t.device)

    expert = gather(fid.expert)
    owner = (expert >= 0).int().argmax(0, keepdim=True)
    pick = lambda t: gather(t).gather(0, owner)[0]  # noqa: E731
    return ops.SampledFidelity(pick(fid.sq_ref), pick(fid.max_ref), pick(fid.sq_err), pick(fid.max_err), pick(fid.range_ref),
                               None, fid.n, fid.rows, expert.gather(0, owner)[0])


def sp_wan_dense(proc, attn, q, k, v, enc_img, is_cross_attn: bool):
    """Dense Wan attention under SP (wan.py:103-149).  Cross attention has replicated K/V (text / image
    tokens): every rank already holds all heads of its query shard and every key, so it needs NO
    communication at all (the reference does an all-to-all of Q and back, wan.py:111-114,147).  The same holds in grad
    mode: `WanAttnProcessor2_0.__call__` takes its local grad path for cross attention and says what a rank ends with."""
    if is_cross_attn:
        return proc._attn(attn, q, k, v, enc_img, True)
    return sp_attention(q, k, v, 0, None, None, model="wan"), None


# ---- the soft mixture (router training) under sequence parallelism -------------------------------------------------------
# After the exchange a rank holds whole heads and the mixture is independent per head: the single-GPU launches
# (routed.soft_mixture_attention) run on the local heads through the receive layout.  Every head costs the same (all three
# experts), so the heads are placed in their natural order: H / P per rank, or -- where P does not divide H -- one more on the
# first H % P ranks (UlyssesLayout(counts=...)).  VORTA_SP_PLACEMENT, VORTA_SP_GROUPS, VORTA_SP_KV_SPLITS and the precision
# switch do not apply: one slot group, one key split, the dtype of q, k, v -- what the single-GPU training forward pins.
# The attention backward is NOT pinned: `backward=` / routed.set_attention_backward / VORTA_ATTENTION_BACKWARD choose among the
# three algorithms as on one GPU (the statistics-based kernels take the receive layout as it is).
def _mixture_placement(H: int, P: int):
    if H < P:
        raise ValueError(f"{H} heads cannot cover {P} sequence-parallel ranks")
    return list(range(H)), [H // P + (1 if j < H % P else 0) for j in range(P)]


def mixture_head_range(H: int):
    """[h0, h1): the heads this rank holds in the sequence-parallel soft mixture (natural order, `_mixture_placement`)"""
    _, counts = _mixture_placement(H, SP_STATE.sp_size)
    me = SP_STATE.group_local_rank
    return sum(counts[:me]), sum(counts[:me + 1])


def _mixture_setup(q, T, model, lowres_group_info, window_size, tile_size, latent_shape):
    B, H, N, D = q.shape
    if B != 1:
        raise AssertionError(f"Batch size {B} is not supported by the sequence-parallel soft mixture.")
    if model != "hunyuan" and T:
        raise ValueError("only the hunyuan model carries text rows in its self attention")
    P, Sl = SP_STATE.sp_size, N - T
    order, counts = _mixture_placement(H, P)
    lay = _layout_only(H, Sl * P, T, D, q.device, q.dtype, counts)
    geom = geometry_for(latent_shape, tile_size, window_size, lowres_group_info.window_size, lowres_group_info.reduction_rate,
                        q.device, row_map=lay.row_map)
    me = SP_STATE.group_local_rank
    return lay, order, geom, (lay.starts[me], lay.starts[me + 1])


def _flat(lay: UlyssesLayout, buf: torch.Tensor) -> torch.Tensor:
    """a receive buffer as ((P + 1) Hl, Sl, D): segment p holds rows of local head p % Hl only (P video chunks, then the text
    segment), so an elementwise per-head kernel sees every row exactly once -- the head views overlap"""
    return buf.view((lay.P + 1) * lay.Hl, lay.Sl, lay.D)


def _recv_mixture_forward(lay, geom, qb, kb, vb, scores, ebufs, ob, model, T, te, scale, record=None):
    """the three experts over the local heads in the receive layout, then the mix: scores (1, Hl, 3)"""
    hv = lay.head_view
    routed_attention(hv(qb), hv(kb), hv(vb), HeadRouting.every_head_everywhere(lay.Hl, qb.device), geom, model=model,
                     text_len=T, text_valid=te, scale=scale, expert_outs=[hv(b) for b in ebufs], fp8=False, kv_splits=1,
                     record=record)
    ops.mix_experts([_flat(lay, b) for b in ebufs], scores[:1].repeat(1, lay.P + 1, 1), _flat(lay, ob))


def _recv_fidelity(lay, ebufs, ob) -> "ops.ExpertFidelity":
    """ops.expert_fidelity of this rank's heads from receive buffers: the kernel sees the (P + 1) Hl segments of `_flat` (every
    row exactly once) and the per-segment results are combined here, as mix_experts_bwd's are: sums add, maxima meet.  A
    head's range would need the segments' signed extremes, which the kernel does not hand out: range_ref is not carried.  A
    sum's chain of roundings is _C.fidelity_chain(Sl) + P here.  The rows of the text segment beyond the text length are
    zero in all four buffers (`new_buffer`, `new_recv_buffer`), and zeros add nothing to a sum or to a maximum of magnitudes."""
    f = ops.expert_fidelity([_flat(lay, b) for b in ebufs], _flat(lay, ob))
    seg = lambda t: t.view(lay.P + 1, lay.Hl, *t.shape[1:])  # noqa: E731
    return ops.ExpertFidelity(seg(f.sq_ref).sum(0), seg(f.max_ref).amax(0), seg(f.sq_err).sum(0), seg(f.max_err).amax(0), None,
                              lay.D * (lay.S + lay.T))


def gather_fidelity(fid: "ops.ExpertFidelity", H: int) -> "ops.ExpertFidelity":
    """this rank's statistics ((..., Hl) / (..., Hl, 3), heads `mixture_head_range(H)`) -> all H heads in head order: one
    all-gather per tensor over the sequence-parallel group, padded to the largest head count (a collective: every rank
    calls it).  A gloo group gathers host copies."""
    import torch.distributed as dist
    P = SP_STATE.sp_size
    _, counts = _mixture_placement(H, P)
    staged = dist.get_backend(SP_STATE.group) == "gloo"

    def gather(t, axis):  # `axis`: the head axis
        pad = t.new_zeros(t.shape[:axis] + (max(counts),) + t.shape[axis + 1:])
        pad.narrow(axis, 0, t.shape[axis]).copy_(t)
        src = pad.cpu() if staged else pad.contiguous()
        parts = [torch.empty_like(src) for _ in range(P)]
        dist.all_gather(parts, src, group=SP_STATE.group)
        return torch.cat([p.narrow(axis, 0, c) for p, c in zip(parts, counts)], dim=axis).to(t.device)

    return ops.ExpertFidelity(gather(fid.sq_ref, fid.sq_ref.dim() - 1), gather(fid.max_ref, fid.max_ref.dim() - 1),
                              gather(fid.sq_err, fid.sq_err.dim() - 2), gather(fid.max_err, fid.max_err.dim() - 2), None, fid.n)


class _RecvSoftMixture(torch.autograd.Function):
    """routed.`_SoftMixture` on receive buffers: q, k, v in, the mixed output out, all (rows_total, D) of one layout"""

    # the list `sp_soft_mixture_attention_autograd(fidelity=...)` hands over for the length of its `apply` (the inputs of
    # `forward` end with the algorithm); a forward recomputed later, under gradient checkpointing, finds None and measures nothing
    fidelity_sink = None

    @staticmethod
    def forward(ctx, qb, kb, vb, scores, lay, geom, model, T, te, scale, backward=None):
        from ..routed import attention_backward
        from ..ulysses.autograd import new_recv_buffer
        ctx.algorithm = attention_backward(backward)  # read when the forward runs, as routed._SoftMixture reads it
        ebufs = [new_recv_buffer(lay) for _ in range(3)]
        ob = new_recv_buffer(lay)
        launches: list = []
        _recv_mixture_forward(lay, geom, qb, kb, vb, scores, ebufs, ob, model, T, te, scale, record=launches)
        if _RecvSoftMixture.fidelity_sink is not None:
            _RecvSoftMixture.fidelity_sink.append(_recv_fidelity(lay, ebufs, ob))
        ctx.save_for_backward(qb, kb, vb, scores, *ebufs)
        from ..routed import _unbind_launches
        ctx.launches, ctx.lay = _unbind_launches(launches, ebufs), lay  # (a head view starts where its buffer starts)
        return ob

    @staticmethod
    def backward(ctx, d_ob):
        from ..routed import _bind_launches, _replay_backward
        qb, kb, vb, scores, *ebufs = ctx.saved_tensors
        lay = ctx.lay
        hv = lay.head_view
        g = d_ob.contiguous()
        dsc = ops.mix_experts_bwd([_flat(lay, b) for b in ebufs], _flat(lay, g)).view(lay.P + 1, lay.Hl, 3).sum(0)
        sc = scores[0].to(qb.dtype).contiguous()  # what ops.mix_experts read in the forward
        ptrs = [b.data_ptr() for b in ebufs]
        # float32 accumulators laid out like the receive buffers: a launch adds through the same row tables and head stride
        acc = [torch.zeros((lay.rows_total, lay.D), dtype=torch.float32, device=qb.device) for _ in range(3)]
        # (the algorithm the forward resolved; the statistics-based kernels take the same row tables and head stride -- what
        # "deterministic" needs of this layout, one writer per accumulator row inside a launch: DESIGN.md 6.8)
        launches = _bind_launches(ctx.launches, hv(qb), hv(kb), hv(vb), [hv(b) for b in ebufs])
        _replay_backward(launches, hv(g), hv(acc[0]), hv(acc[1]), hv(acc[2]),
                         lambda _, o: sc[:, ptrs.index(o.data_ptr())], algorithm=ctx.algorithm)
        grads = [torch.empty_like(qb) for _ in range(3)]
        ops.cast_grads([_flat(lay, a) for a in acc], [_flat(lay, x) for x in grads])
        d_sc = torch.zeros_like(scores)
        d_sc[0] = dsc.to(scores.dtype)
        return grads[0], grads[1], grads[2], d_sc, None, None, None, None, None, None, None


def sp_soft_mixture_attention(q, k, v, T: int, routing_score: torch.Tensor, *, model: str, text_valid: int = 0,
                              lowres_group_info=None, window_size=(3, 3, 3), tile_size=(6, 8, 8), latent_shape=None,
                              scale: Optional[float] = None, fidelity: Optional[list] = None) -> torch.Tensor:
    """`routed.soft_mixture_attention` under sequence parallelism, forward only (no autograd graph).
    q,k,v: (1, H, S/P + T, D) local sequence shard with the replicated text at the end, as `sp_attention`; routing_score
    (B, H, 3), item 0 is read.  Returns the (1, S/P + T, H, D) buffer (text rows: all heads, gathered).  The receive
    buffers are the cached ones of the inference path.
    fidelity: a list that receives one `ops.ExpertFidelity` of THIS RANK's heads [h0, h1) (`mixture_head_range`), over
    their whole sequences; the caller gathers across ranks.  None: launches and bits are unchanged."""
    with torch.no_grad():
        lay, order, geom, (h0, h1) = _mixture_setup(q, T, model, lowres_group_info, window_size, tile_size, latent_shape)
        _, sb = _layout(lay.H, lay.S, T, lay.D, q.device, q.dtype, lay.counts)
        if getattr(sb, "mix_bufs", None) is None:
            sb.mix_bufs = [lay.new_buffer() for _ in range(3)]  # the three experts' outputs, beside q, k, v, o
        Sl = lay.Sl
        lay.scatter_heads([x[0, :, :Sl] for x in (q, k, v)], sb.bufs[:3], order, [x[0, :, Sl:] for x in (q, k, v)] if T else None)
        te = text_valid if model == "hunyuan" else 0
        _recv_mixture_forward(lay, geom, *sb.bufs[:3], routing_score[:1, h0:h1], sb.mix_bufs, sb.bufs[3], model, T, te, scale)
        if fidelity is not None:
            fidelity.append(_recv_fidelity(lay, sb.mix_bufs, sb.bufs[3]))
        buf = torch.empty((1, Sl + T, lay.H, lay.D), dtype=q.dtype, device=q.device)
        lay.gather_heads(sb.bufs[3], buf[0, :Sl].transpose(0, 1), order, buf[0, Sl:].transpose(0, 1) if T else None)
        return buf


def sp_soft_mixture_attention_autograd(q, k, v, T: int, routing_score: torch.Tensor, *, model: str, text_valid: int = 0,
                                       lowres_group_info=None, window_size=(3, 3, 3), tile_size=(6, 8, 8),
                                       latent_shape=None, scale: Optional[float] = None,
                                       backward: Optional[str] = None, fidelity: Optional[list] = None) -> torch.Tensor:
    """`sp_soft_mixture_attention` as a differentiable operator (`routed.soft_mixture_attention_autograd` on the local heads
    between a differentiable exchange, ulysses/autograd.py).  The backward exchanges d_out to head shards, takes the score
    gradients (ops.mix_experts_bwd), replays the recorded launches into float32 buffers laid out like the receive buffers,
    rounds once (ops.cast_grads) and sends dq, dk, dv back in one exchange.  Text rows of dq, dk, dv and
    d routing_score are non-zero for this rank's heads only: their sum over the ranks is the single-process gradient.
    Every buffer an autograd node keeps is allocated by this call (the next layer overwrites the shared ones).
    `backward`: "query_major" (ops.attn_bwd), "key_major" (ops.attn_bwd_stats + ops.attn_bwd_key_major) or "deterministic"
    (ops.attn_bwd_stats + ops.attn_bwd_dq + ops.attn_bwd_dkv: no float atomic -- on every rank dq, dk, dv and the score
    gradients repeat bit for bit; a sum ACROSS ranks, the training loop's all-reduce of text-row and score
    gradients, is outside that claim), as for `routed.soft_mixture_attention_autograd`; None follows
    `routed.set_attention_backward` / VORTA_ATTENTION_BACKWARD, else "query_major".  It is resolved when the forward runs,
    and an unknown name is refused before a layout is built or a collective runs.  The forward is the same whichever it is.
    `fidelity`: as for `sp_soft_mixture_attention` (this rank's heads; no gradient flows through it)."""
    from ..routed import attention_backward
    from ..ulysses.autograd import gather_heads_autograd, scatter_heads_autograd
    algorithm = attention_backward(backward)
    lay, order, geom, (h0, h1) = _mixture_setup(q, T, model, lowres_group_info, window_size, tile_size, latent_shape)
    qb, kb, vb = scatter_heads_autograd(lay, [q[0], k[0], v[0]], order)
    te = text_valid if model == "hunyuan" else 0
    previous, _RecvSoftMixture.fidelity_sink = _RecvSoftMixture.fidelity_sink, fidelity
    try:
        ob = _RecvSoftMixture.apply(qb, kb, vb, routing_score[:1, h0:h1], lay, geom, model, T, te, scale, algorithm)
    finally:
        _RecvSoftMixture.fidelity_sink = previous
    return gather_heads_autograd(lay, ob, order, token_major=True)[None]
