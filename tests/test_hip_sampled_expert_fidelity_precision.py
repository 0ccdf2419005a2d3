"""GPU: `routed.sampled_expert_fidelity(precision="fp8pv" | "i8pv")` -- the per-expert measurement IN a tier's precision.

Fixtures of tests/test_hip_routed_fidelity.py: latent (8,6,8), S = 384, H = 6, both models; no key list reaches 16 key blocks,
so no launch cuts its keys.

(1) The three compact candidate buffers (`outputs=`: coreset, sliding tile, full attention in the tier) against the sampled
rows of the full-size expert outputs under that precision (`routed_attention(every_head_everywhere, expert_outs=..., fp8=p)`).
"fp8pv": `torch.equal` -- the 16-bit-score kernel treats every query row on its own.  "i8pv": NOT bit equal, for a structural
reason: the int8-score kernel quantises a wave's 32 query rows with ONE scale, the wave's own (csrc/attn_fwd_i8.hip: "one
query scale per WAVE (sq, taken by the wave itself over its 32 rows)"), and the compact launch groups the sampled rows into
other waves than the full-size launch does; DESIGN.md 6.8 states it.  Those rows are held instead to 2 x the error of the
full-size "i8pv" output against the float64 oracle, per head and candidate.
(2) The record against a float64 evaluation of the compact buffers, at the chain bound of vorta_expert_fidelity, as the native
test holds it.  (3) The dense column (sq_ref, max_ref, range_ref, and the reference buffer) equals the native call's."""
import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O
from test_hip_routed_fidelity import GROUP, H, LATENT, TILE, WINDOW, _geom, _inputs, _text
from test_hip_sampled_expert_fidelity import _check_record
from _util import dev

pytestmark = pytest.mark.gpu

S, SEED = 384, 3
_FULL, _ORACLE = {}, {}


def _full_experts(model, precision):
    """the three full-size expert outputs (H, S + T, D) of every head under `precision`, computed once"""
    from vorta_amd.routed import HeadRouting, routed_attention
    key = (model, precision)
    if key not in _FULL:
        q, k, v, _ = _inputs(model)
        T, te = _text(model)
        bufs = [torch.empty_like(q) for _ in range(3)]
        routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, dev()), _geom(), model=model, text_len=T, text_valid=te,
                         expert_outs=bufs, fp8=precision)
        torch.cuda.synchronize()
        _FULL[key] = [b[0] for b in bufs]
    return _FULL[key]


def _oracle_experts(model):
    """the float64 oracle's three expert outputs (H, S + T, D), computed once"""
    if model not in _ORACLE:
        q, k, v, _ = _inputs(model)
        T, te = _text(model)
        gi = O.group_info(LATENT, GROUP, 0.5)
        x = [t.double().cpu().numpy() for t in (q, k, v)]
        _ORACLE[model] = [O.routed_attention(*x, np.full(H, e), model=model, latent=LATENT, tile=TILE, window=WINDOW, gi=gi,
                                             t_text=T, t_eff=te)[0] for e in range(3)]
    return _ORACLE[model]


@pytest.mark.parametrize("n", [S, 96])
@pytest.mark.parametrize("precision", ["fp8pv", "i8pv"])
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_candidate_rows_record_and_dense_column(model, precision, n):
    from vorta_amd.routed import sample_rows, sampled_expert_fidelity
    q, k, v, _ = _inputs(model)
    T, te = _text(model)
    geom = _geom()
    kw = dict(model=model, text_len=T, text_valid=te, rows=n, seed=SEED)
    native_outs, outs = [], []
    native = sampled_expert_fidelity(q, k, v, geom, outputs=native_outs, **kw)
    fid = sampled_expert_fidelity(q, k, v, geom, outputs=outs, precision=precision, **kw)
    assert len(outs) == 5 and torch.equal(outs[-1], native_outs[-1])
    tokens = sample_rows(S, n, SEED, dev())[outs[-1]].long()
    full = _full_experts(model, precision)
    # (1) coreset, sliding tile, full attention in the tier: outs[1], outs[2], outs[3] against experts 1, 2, 0
    for name, got, e in (("coreset", outs[1], 1), ("sliding", outs[2], 2), ("full", outs[3], 0)):
        want = full[e][:, tokens]
        if precision == "fp8pv":
            bad = (got != want).any(-1).nonzero().tolist()[:4]
            assert torch.equal(got, want), f"{model} fp8pv n={n}: {name} rows differ from the full-size launch at (head, position) {bad}"
            continue
        oracle = torch.from_numpy(_oracle_experts(model)[e]).to(dev())[:, tokens]
        err_rows = (got.double() - oracle).pow(2).sum((1, 2)).sqrt()
        err_full = (want.double() - oracle).pow(2).sum((1, 2)).sqrt()
        print(f"{model} i8pv n={n} {name}: compact / full-size error against float64 per head "
              f"{[round(float(a / b), 3) for a, b in zip(err_rows, err_full)]}; bit-equal rows "
              f"{int((got == want).all(-1).sum())} of {got.shape[0] * got.shape[1]}")
        assert bool((err_rows <= 2.0 * err_full).all()), (model, n, name, err_rows.tolist(), err_full.tolist())
    # (2) the record is the float64 evaluation of the buffers, to the chain bound; column 2 is the tier's full attention
    _check_record(fid, outs, range(H), True, f"{model} {precision} n = {n}")
    rel = fid.rel_error()
    assert bool(torch.isfinite(rel).all()) and bool((rel > 0).all()), rel  # 8 bits cost every candidate something
    # (3) the dense reference stays in the input dtype: the native call's bits
    assert torch.equal(outs[0], native_outs[0])
    for name in ("sq_ref", "max_ref", "range_ref"):
        assert torch.equal(getattr(fid, name), getattr(native, name)), name
    assert fid.n == native.n


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_operands_are_reused_and_auto8_operands_serve_both_tiers(model, monkeypatch):
    """`operands=`: nothing is converted again, and the record has the bits of the call that converted its own; the operands of
    "auto8" hold both tiers' key sides; a head list leaves the other heads NaN"""
    import vorta_amd.routed as rt
    from vorta_amd.routed import prepare_operands, sampled_expert_fidelity
    q, k, v, _ = _inputs(model)
    T, te = _text(model)
    geom = _geom()
    kw = dict(model=model, text_len=T, text_valid=te, rows=96, seed=SEED)
    own = {p: sampled_expert_fidelity(q, k, v, geom, precision=p, **kw) for p in ("fp8pv", "i8pv")}
    prepared = {p: prepare_operands(p, q[0], k[0], v[0], None) for p in ("fp8pv", "i8pv", "auto8")}
    calls = []
    monkeypatch.setattr(rt, "prepare_operands", lambda *a, **k_: calls.append(a[0]))
    for p in ("fp8pv", "i8pv"):
        for given in (p, "auto8"):
            fid = sampled_expert_fidelity(q, k, v, geom, precision=p, operands=prepared[given], **kw)
            for name in ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref"):
                assert torch.equal(getattr(fid, name), getattr(own[p], name)), (p, given, name)
    assert calls == []
    monkeypatch.undo()
    part = sampled_expert_fidelity(q, k, v, geom, precision="i8pv", heads=[4, 1], **kw)
    assert torch.isfinite(part.sq_err).all(-1).tolist() == [h in (1, 4) for h in range(H)]
    assert torch.equal(part.sq_err[[1, 4]], own["i8pv"].sq_err[[1, 4]])


def test_refusals():
    from vorta_amd.routed import prepare_operands, sampled_expert_fidelity
    q, k, v, _ = _inputs("wan")
    geom = _geom()
    with pytest.raises(ValueError, match="precision= together with out="):
        sampled_expert_fidelity(q, k, v, geom, model="wan", rows=48, precision="i8pv", out=torch.empty_like(q))
    for bad in ("auto8", "native", "fp8", "int4"):
        with pytest.raises(ValueError, match="precision="):
            sampled_expert_fidelity(q, k, v, geom, model="wan", rows=48, precision=bad)
    with pytest.raises(ValueError, match="operands= goes with precision="):
        sampled_expert_fidelity(q, k, v, geom, model="wan", rows=48, operands=prepare_operands("i8pv", q[0], k[0], v[0], None))
    with pytest.raises(ValueError, match="operands of 'fp8pv'"):
        sampled_expert_fidelity(q, k, v, geom, model="wan", rows=48, precision="i8pv",
                                operands=prepare_operands("fp8pv", q[0], k[0], v[0], None))
