"""GPU parity of the fp8 (e4m3) path -- BASELINE.json configs[4] "fp8 MFMA QK^T/PV path" -- through the C ABI
(vorta_fp8_quantize_qkv, vorta_attn_fwd_fp8, vorta_attn_fwd_batch_fp8).

The reference has no fp8 code, so the gates are this build's own, stated here and in DESIGN.md:
  gate (i)   kernel vs the oracle's emulator (oracle/vorta_oracle.py: fp8_attn_launch) on the SAME e4m3 operands,
             with the probabilities rounded to e4m3 at the same reference points: the existing 16-bit tolerances
             (tests/_util.py ATOL_SAME / RELF_SAME of the OUTPUT dtype) -- what is left is fp32 accumulation.
             A probability within fp32 noise (1e-4 relative; flips observed up to 5e-5) of an e4m3 rounding midpoint may legitimately round the
             other way; the emulator returns, per row, the normalised mass `a` of those probabilities, and the row's
             tolerance grows by 2^-3 * a * 2 max|v| (each of them moving one e4m3 step); `a` is 0 for most rows and
             ~1e-3 otherwise.  Waves whose reference point itself is in doubt (a block max within 1e-4 of `defer`) are
             skipped (none in these tests but for a handful of rows);
  gate (i')  kernel vs exact softmax attention on the dequantised operands (no probability rounding): the cost of
             packing P to e4m3, bounded at rel. Frobenius <= 3e-2;
  gate (ii)  operator PSNR >= 40 dB against the bf16 kernel on the 16-bit inputs, Wan-14B-81f geometry, each expert:
             10 log10(R^2 / mse) with R = the data range max - min of the bf16 output (the convention of
             skimage.metrics.peak_signal_noise_ratio / torchmetrics for float data).  The stricter figure with
             R = max |output| (6 dB lower for a symmetric signal) is printed beside it and held above 39 dB.  The inputs
             are white noise (no structure for the quantisation noise to average against): the worst case for the
             rounding noise, the best case for the operand ranges -- keys with a common component (a per-channel mean)
             fall under the gate unless the conversion centres them, which it does by default (flags bit1).
"""
import math

import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O

pytestmark = pytest.mark.gpu

from _util import ATOL_SAME, RELF_SAME, dev, rel_fro, rounded, to_dev  # noqa: E402

RELF_PACK = 3e-2  # gate (i')


def _decoded(f8):
    """the GPU's e4m3 operands as float64 (H,S,D) arrays + v_descale (H,D)"""
    return (O.e4m3_decode(f8.q.cpu().numpy()), O.e4m3_decode(f8.k.cpu().numpy()), O.e4m3_decode(f8.v.cpu().numpy()),
            f8.v_descale.cpu().numpy().astype(np.float64))


def _psnr(x, ref):
    """(PSNR over the data range max - min, PSNR over max |ref|, relative rms error)"""
    x, ref = x.float(), ref.float()
    mse = torch.mean((x - ref) ** 2).item()
    rng, peak = (ref.max() - ref.min()).item(), ref.abs().max().item()
    f = lambda r: 10.0 * math.log10(r * r / max(mse, 1e-30))
    return f(rng), f(peak), math.sqrt(mse / torch.mean(ref ** 2).item())


def _vmax(v8, vd):
    return float(np.abs(v8 * vd[:, None, :]).max())


def _bits(x):
    return x.contiguous().view(torch.int16)


def _check(out, ref, dtype, amb, vmax):
    """amb: the emulator's per-row normalised mass of probabilities within fp32 noise of a rounding midpoint (inf =
    reference point in doubt); vmax = max |v * v_descale|"""
    out = out.float().cpu().numpy().reshape(-1, ref.shape[-1])
    ref = ref.reshape(-1, ref.shape[-1])
    amb = amb.reshape(-1)
    ok = np.isfinite(amb)
    assert ok.mean() >= 0.9, f"{(~ok).sum()} of {ok.size} rows have a reference point in doubt"
    out, ref, amb = out[ok], ref[ok], amb[ok]
    tol = ATOL_SAME[dtype] + 0.125 * amb * 2 * vmax
    err = np.abs(out - ref).max(1)
    assert (err <= tol).all(), f"max|d|={err.max():.3e} at slack {amb[err.argmax()]:.2e} (tol {tol[err.argmax()]:.3e})"
    assert np.median(amb) < 1e-2
    rf = rel_fro(out, ref)
    assert rf <= RELF_SAME[dtype] + 0.125 * float(np.sqrt((amb ** 2).mean())) * 4, f"relF={rf:.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantizer_matches_oracle_bit_for_bit(dtype):
    from vorta_amd import ops
    rng = np.random.default_rng(0)
    H, S = 3, 1500
    q = rng.standard_normal((H, S, 128)) * np.array([0.5, 1.0, 6.0])[:, None, None]
    k = rng.standard_normal((H, S, 128)) * np.array([2.0, 1.0, 0.3])[:, None, None]
    v = rng.standard_normal((H, S, 128)) * np.linspace(0.05, 8.0, 128)
    qd, kd, vd = to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype)
    f8 = ops.fp8_quantize_qkv(qd, kd, vd)
    torch.cuda.synchronize()
    z = O.fp8_quantize_qkv(rounded(q, dtype), rounded(k, dtype), rounded(v, dtype))
    qm, km, vm = (t.cpu().numpy() for t in f8.multipliers())
    assert (qm == z["qmul"]).all() and (km == z["kmul"]).all() and (vm == z["vmul"]).all()
    assert (f8.v_descale.cpu().numpy() == z["v_descale"]).all()
    for name, t in (("q8", f8.q), ("k8", f8.k), ("v8", f8.v)):
        assert (t.cpu().numpy() == z[name]).all(), name
    # strided inputs ((S,H,D) storage) give the same bytes
    packed = torch.stack([qd, kd, vd]).permute(0, 2, 1, 3).contiguous()  # (3,S,H,D)
    g8 = ops.fp8_quantize_qkv(*(packed[i].permute(1, 0, 2) for i in range(3)))
    assert torch.equal(g8.q, f8.q) and torch.equal(g8.k, f8.k) and torch.equal(g8.v, f8.v)
    # one scale per head for v
    h8 = ops.fp8_quantize_qkv(qd, kd, vd, v_per_head=True)
    zh = O.fp8_quantize_qkv(rounded(q, dtype), rounded(k, dtype), rounded(v, dtype), v_per_head=True)
    assert (h8.v.cpu().numpy() == zh["v8"]).all() and (h8.v_descale.cpu().numpy() == zh["v_descale"]).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantizer_key_centring_and_segmented_rows(dtype):
    """flags bit1 (centre the keys) and the Ulysses row layout (seg_len > 0: per-head scales / centres on ONE row array,
    gaps behind the text rows skipped) against the oracle and against the (H,S,D) call on the same data"""
    from vorta_amd import ops
    rng = np.random.default_rng(5)
    Hl, P, Sl, T = 3, 4, 700, 33
    S = P * Sl
    q = rng.standard_normal((Hl, S + T, 128)) * np.array([0.5, 1.0, 4.0])[:, None, None]
    k = rng.standard_normal((Hl, S + T, 128)) + 5.0 * rng.standard_normal((Hl, 1, 128))
    v = rng.standard_normal((Hl, S + T, 128)) * np.linspace(0.05, 8.0, 128)
    qd, kd, vd = to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype)
    kr = rounded(k, dtype)
    # (H,S,D) layout, centred: the centre is the mean of the oracle's sample rows; everything else bit for bit
    # (`video_tokens`: the sample is summed in eighths of the video tokens + the text tokens, in either layout)
    f8 = ops.fp8_quantize_qkv(qd, kd, vd, center_k=True, video_tokens=S)
    c = f8.k_center().cpu().numpy()
    rows = O.fp8_center_rows(S + T, Hl)
    want = np.stack([kr[h, rows[h]].mean(0) for h in range(Hl)])
    assert np.abs(c - want).max() <= 1e-5 * np.abs(want).max()
    z = O.fp8_quantize_qkv(rounded(q, dtype), kr, rounded(v, dtype), k_center=c)
    qm, km, vm = (t.cpu().numpy() for t in f8.multipliers())
    assert (qm == z["qmul"]).all() and (km == z["kmul"]).all() and (vm == z["vmul"]).all()
    for name, t in (("q8", f8.q), ("k8", f8.k), ("v8", f8.v)):
        assert (t.cpu().numpy() == z[name]).all(), name
    assert float(km.max()) > 1.5 * float(ops.fp8_quantize_qkv(qd, kd, vd).multipliers()[1].max())  # the range went to the signal
    # the same data in the receive layout of rank-local heads: chunk j = (Hl, Sl, D), text rows behind slot i's video rows
    rows_video, rows_total = P * Hl * Sl, P * Hl * Sl + Hl * Sl
    phys = lambda h, s: (s // Sl) * Hl * Sl + h * Sl + s % Sl
    bufs = []
    for x in (qd, kd, vd):
        b = torch.full((rows_total, 128), 300.0, dtype=dtype, device=dev())  # gaps hold junk that must not be read
        for h in range(Hl):
            for j in range(P):
                b[phys(h, j * Sl):phys(h, j * Sl) + Sl] = x[h, j * Sl:(j + 1) * Sl]
            b[rows_video + h * Sl:rows_video + h * Sl + T] = x[h, S:]
        bufs.append(b.view(1, rows_total, 128))
    for center in (False, True):
        nws_ = ops._C.lib().vorta_fp8_quant_ws_floats(Hl, 128)
        zero = ops.Fp8Operands(*(torch.zeros((1, rows_total, 128), dtype=torch.uint8, device=dev()) for _ in range(3)),
                               torch.zeros((Hl, 128), dtype=torch.float32, device=dev()),
                               torch.zeros(nws_, dtype=torch.float32, device=dev()))  # gap rows stay zero: comparable
        g8 = ops.fp8_quantize_qkv(*bufs, heads=Hl, seg_len=Sl, tail_first=rows_video, tail_len=T, center_k=center, out=zero)
        cs = g8.k_center().cpu().numpy()
        if center:
            srows = O.fp8_center_rows(rows_total, Hl, Sl, rows_video, T)
            kb = bufs[1][0].float().cpu().numpy()
            want = np.stack([kb[srows[h]].mean(0) for h in range(Hl)])
            assert np.abs(cs - want).max() <= 1e-5 * np.abs(want).max()
        zs = O.fp8_quantize_qkv(rounded(q, dtype), kr, rounded(v, dtype), k_center=cs if center else None)
        qm, km, vm = (t.cpu().numpy() for t in g8.multipliers())
        assert (qm == zs["qmul"]).all() and (km == zs["kmul"]).all() and (vm == zs["vmul"]).all()
        assert (g8.v_descale.cpu().numpy() == zs["v_descale"]).all()
        for name, t in (("q8", g8.q), ("k8", g8.k), ("v8", g8.v)):
            got = t[0].cpu().numpy()
            for h in range(Hl):
                for j in range(P):
                    assert (got[phys(h, j * Sl):phys(h, j * Sl) + Sl] == zs[name][h, j * Sl:(j + 1) * Sl]).all(), (name, h, j)
                assert (got[rows_video + h * Sl:rows_video + h * Sl + T] == zs[name][h, S:]).all(), (name, h, "text")
        if center:  # the same TOKENS define the centre in both layouts: same centre, same bytes as the (H,S,D) call
            assert (cs == c).all()
            for name, t, u in (("q8", g8.q, f8.q), ("k8", g8.k, f8.k), ("v8", g8.v, f8.v)):
                got = t[0]
                for h in range(Hl):
                    for j in range(P):
                        assert torch.equal(got[phys(h, j * Sl):phys(h, j * Sl) + Sl], u[h, j * Sl:(j + 1) * Sl]), (name, h, j)
        # slot group by slot group (the overlapped exchange converts the group that has landed): the bytes of one call
        nws = g8.ws.numel()
        part = ops.Fp8Operands(*(torch.zeros_like(t) for t in (g8.q, g8.k, g8.v)), torch.zeros_like(g8.v_descale),
                               torch.zeros(nws, dtype=torch.float32, device=dev()))
        for slots in ((2, 3), (0, 2)):
            ops.fp8_quantize_qkv(*bufs, heads=Hl, seg_len=Sl, tail_first=rows_video, tail_len=T, center_k=center,
                                 out=part, slots=slots)
        for name in ("q", "k", "v", "v_descale"):
            assert torch.equal(getattr(part, name), getattr(g8, name)), (name, center)
        # v converted on the SEND side of the exchange: abs-max of every sequence shard (+ the replicated text rows),
        # MAX over the shards, conversion into destination head order -- the receive-side bytes and v_descale
        order = [2, 0, 1]
        omap = torch.tensor(order, dtype=torch.int32, device=dev())
        amax_parts = []
        for j in range(P):
            am = torch.zeros((Hl, 128), dtype=torch.float32, device=dev())
            ops.fp8_v_absmax(vd[:, j * Sl:(j + 1) * Sl], am)
            ops.fp8_v_absmax(vd[:, S:], am)
            amax_parts.append(am)
        amax = torch.stack(amax_parts).amax(0)  # the all-reduce
        assert torch.equal(amax, vd.float().abs().amax(1))
        for j in range(P):
            st = torch.empty((Hl, Sl, 128), dtype=torch.uint8, device=dev())
            vdsc = torch.empty((Hl, 128), dtype=torch.float32, device=dev())
            ops.fp8_v_convert(vd[:, j * Sl:(j + 1) * Sl], amax, st, src_map=omap, v_descale=vdsc)
            assert torch.equal(vdsc, g8.v_descale[omap.long()])
            for i, h in enumerate(order):
                assert torch.equal(st[i], g8.v[0, phys(h, j * Sl):phys(h, j * Sl) + Sl]), (j, h)
        tx = torch.empty((Hl, T, 128), dtype=torch.uint8, device=dev())
        ops.fp8_v_convert(vd[:, S:], amax, tx)
        for h in range(Hl):
            assert torch.equal(tx[h], g8.v[0, rows_video + h * Sl:rows_video + h * Sl + T])
        # q and k only (v arrived as e4m3): v / v_descale of the operand set are left alone
        qk = ops.Fp8Operands(torch.zeros_like(g8.q), torch.zeros_like(g8.k), torch.full_like(g8.v, 7),
                             torch.full_like(g8.v_descale, 3.0), torch.zeros(nws, dtype=torch.float32, device=dev()))
        ops.fp8_quantize_qkv(bufs[0], bufs[1], None, heads=Hl, seg_len=Sl, tail_first=rows_video, tail_len=T,
                             center_k=center, out=qk)
        assert torch.equal(qk.q, g8.q) and torch.equal(qk.k, g8.k) and bool((qk.v == 7).all()) and bool((qk.v_descale == 3.0).all())
    with pytest.raises(ValueError):
        ops.fp8_quantize_qkv(qd, kd, vd, seg_len=Sl)  # segmented layout needs (1,rows,D) arrays and `heads`
    with pytest.raises(ValueError):
        ops.fp8_quantize_qkv(qd, kd, vd, slots=(0, 1))  # a slot range needs the segmented layout
    with pytest.raises(ValueError):  # VORTA_EINVAL: the text region starts on a segment boundary
        ops.fp8_quantize_qkv(*bufs, heads=Hl, seg_len=Sl, tail_first=rows_video + 1, tail_len=T)


def test_key_centring_buys_back_a_common_key_component():
    """keys with a per-channel mean of 8 standard deviations: the e4m3 operator falls under the 40 dB gate without the
    centring and keeps its white-noise PSNR with it (what `routed_attention(fp8=True)` does by default)"""
    from vorta_amd import ops
    H, S = 2, 8192
    g = torch.Generator(device=dev()).manual_seed(11)
    q = torch.randn((H, S, 128), generator=g, device=dev()).to(torch.bfloat16)
    k = (torch.randn((H, S, 128), generator=g, device=dev()) +
         8.0 * torch.randn((H, 1, 128), generator=g, device=dev())).to(torch.bfloat16)
    v = torch.randn((H, S, 128), generator=g, device=dev()).to(torch.bfloat16)
    ref = torch.empty_like(q)
    ops.attn_fwd(q, k, v, ref, n_q=S, n_kv=S)
    res = {}
    for center in (False, True):
        f8 = ops.fp8_quantize_qkv(q, k, v, center_k=center)
        o = torch.empty_like(q)
        ops.attn_fwd(f8.q, f8.k, f8.v, o, n_q=S, n_kv=S, v_descale=f8.v_descale)
        res[center] = _psnr(o, ref)
    print("fp8 vs bf16, keys with an 8-sigma common component (PSNR range dB, PSNR peak dB, rel rms): as is",
          tuple(round(x, 3) for x in res[False]), "centred", tuple(round(x, 3) for x in res[True]))
    assert res[True][0] >= 40.0 and res[False][0] < 40.0 and res[True][0] >= res[False][0] + 8.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("lsum_valu", [0, 1])
def test_fp8_dense_ragged_vs_emulator(dtype, block_rows, lsum_valu):
    """(the rows past q_valid are zero BITS: v is Gaussian, so about half of the accumulators there are negative, and an
    epilogue that multiplies them by 0 instead of selecting on the position writes -0 in those rows)"""
    from vorta_amd import ops
    rng = np.random.default_rng(1)
    H, Sq, Skv = 3, 333, 417
    q, k, v = rng.standard_normal((H, Sq, 128)), rng.standard_normal((H, Skv, 128)), rng.standard_normal((H, Skv, 128))
    n_kv, q_valid = 401, 300
    pad = np.zeros((H, Skv - Sq, 128))
    f8 = ops.fp8_quantize_qkv(to_dev(np.concatenate([q, pad], 1), dtype), to_dev(k, dtype), to_dev(v, dtype))
    out = torch.full((H, Sq, 128), 7.0, dtype=dtype, device=dev())
    ops.attn_fwd(f8.q[:, :Sq], f8.k, f8.v, out, n_q=Sq, n_kv=n_kv, q_valid=q_valid, block_rows=block_rows,
                 v_descale=f8.v_descale, fp8_opts=dict(flags=lsum_valu))
    torch.cuda.synchronize()
    q8, k8, v8, vd = _decoded(f8)
    ref, exact, amb = np.zeros((H, Sq, 128)), np.zeros((H, Sq, 128)), np.zeros((H, Sq))
    for h in range(H):
        if not lsum_valu:
            O.fp8_attn_launch(q8[h], k8[h], v8[h], ref[h], vd[h], n_q=Sq, n_kv=n_kv, q_valid=q_valid, ambiguous=amb[h])
        O.fp8_attn_launch(q8[h], k8[h], v8[h], exact[h], vd[h], n_q=Sq, n_kv=n_kv, q_valid=q_valid, round_p=False)
    if not lsum_valu:  # the VALU row sum adds the UNrounded P: not what the emulator models; gate (i') only
        _check(out, ref, dtype, amb, _vmax(v8, vd))
    assert rel_fro(out.float().cpu().numpy(), exact) <= RELF_PACK
    assert not _bits(out[:, q_valid:]).any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp8_rows_past_q_valid_are_zeros_whatever_q_holds(dtype):
    """include/vorta_hip.h: positions at or past q_valid "are written as zeros".  The ragged shape above in 256-row
    workgroups: q_valid = 300 cuts the wave of positions 288 .. 319, and the rows 300 .. 319 of head 0 hold the e4m3 NaN
    (byte 0x7F) in every channel of q, so their accumulators are NaN.  The output there is zero bits (0 x NaN would be NaN),
    everything below q_valid is finite, and what no NaN row shares a wave with -- positions below 288 of head 0, heads 1 and
    2 -- is bit-equal to the launch with clean q (waves share no state).  The rows 288 .. 299 share the cut wave's rescale
    decisions and are only required to be finite."""
    from vorta_amd import ops
    rng = np.random.default_rng(1)
    H, Sq, Skv = 3, 333, 417
    q, k, v = rng.standard_normal((H, Sq, 128)), rng.standard_normal((H, Skv, 128)), rng.standard_normal((H, Skv, 128))
    n_kv, q_valid = 401, 300
    pad = np.zeros((H, Skv - Sq, 128))
    f8 = ops.fp8_quantize_qkv(to_dev(np.concatenate([q, pad], 1), dtype), to_dev(k, dtype), to_dev(v, dtype))
    q_nan = f8.q.clone()
    q_nan[0, 300:320] = 0x7F
    outs = []
    for q8 in (f8.q, q_nan):
        out = torch.full((H, Sq, 128), 7.0, dtype=dtype, device=dev())
        ops.attn_fwd(q8[:, :Sq], f8.k, f8.v, out, n_q=Sq, n_kv=n_kv, q_valid=q_valid, block_rows=256, v_descale=f8.v_descale)
        outs.append(out)
    torch.cuda.synchronize()
    clean, got = outs
    assert not _bits(got[:, q_valid:]).any(), "rows past q_valid are not zero bits"
    assert torch.isfinite(got[:, :q_valid].float()).all()
    assert torch.equal(_bits(got[0, :288]), _bits(clean[0, :288])) and torch.equal(_bits(got[1:]), _bits(clean[1:]))


def test_fp8_rescale_branch_and_long_keys():
    """key norms grow along the sequence: the reference point of every wave moves several times"""
    from vorta_amd import ops
    dtype = torch.float16
    rng = np.random.default_rng(2)
    H, Sq, Skv = 2, 96, 2048
    q = rng.standard_normal((H, Skv, 128))
    k = rng.standard_normal((H, Skv, 128)) * np.linspace(0.3, 3.0, Skv)[None, :, None]
    v = rng.standard_normal((H, Skv, 128))
    f8 = ops.fp8_quantize_qkv(to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype))
    out = torch.empty((H, Sq, 128), dtype=dtype, device=dev())
    ops.attn_fwd(f8.q[:, :Sq], f8.k, f8.v, out, n_q=Sq, n_kv=Skv, v_descale=f8.v_descale)
    q8, k8, v8, vd = _decoded(f8)
    ref, amb = np.zeros((H, Sq, 128)), np.zeros((H, Skv))
    moved = 0
    for h in range(H):
        O.fp8_attn_launch(q8[h], k8[h], v8[h], ref[h], vd[h], n_q=Sq, n_kv=Skv, ambiguous=amb[h])
        _, _, m = O._fp8_flash_rows(q8[h, :32], k8[h], v8[h], 0, Skv // 64, 5.0, 3.0, True)
        moved += int((m > (q8[h, :32] @ k8[h, :64].T).max(1)).sum())
    assert moved > 0
    _check(out, ref, dtype, amb[:, :Sq], _vmax(v8, vd))
    # other (p_bias, defer) splits of the e4m3 range follow the emulator too
    for pb, df in ((6.0, 2.0), (2.0, 6.0)):
        ops.attn_fwd(f8.q[:, :Sq], f8.k, f8.v, out, n_q=Sq, n_kv=Skv, v_descale=f8.v_descale,
                     fp8_opts=dict(p_bias=pb, defer=df))
        amb[:] = False
        for h in range(H):
            O.fp8_attn_launch(q8[h], k8[h], v8[h], ref[h], vd[h], n_q=Sq, n_kv=Skv, p_bias=pb, defer=df, ambiguous=amb[h])
        _check(out, ref, dtype, amb[:, :Sq], _vmax(v8, vd))
    with pytest.raises(ValueError):
        ops.attn_fwd(f8.q[:, :Sq], f8.k, f8.v, out, n_q=Sq, n_kv=Skv, v_descale=f8.v_descale,
                     fp8_opts=dict(p_bias=6.0, defer=3.0))  # P' could reach 2^9 > 448


@pytest.mark.parametrize("block_rows", [128, 256])
def test_fp8_tables_groups_duplicates_heads(block_rows):
    from vorta_amd import ops
    dtype = torch.bfloat16
    rng = np.random.default_rng(3)
    H, rows = 4, 700
    x = [rng.standard_normal((H, rows, 128)) for _ in range(3)]
    f8 = ops.fp8_quantize_qkv(*(to_dev(a, dtype) for a in x))
    n_q, glen, n_kv = 520, 200, 391  # 3 groups (200, 200, 120), own key list per group
    q_rows = rng.permutation(rows)[:n_q].astype(np.int32)
    kv_rows = np.stack([rng.permutation(rows)[:n_kv] for _ in range(3)]).astype(np.int32)
    free = np.setdiff1d(np.arange(rows), q_rows)
    dup = rng.permutation(free)[:2 * 60].reshape(60, 2).astype(np.int32)
    heads = torch.tensor([3, 0, 2], dtype=torch.int32, device=dev())
    count = torch.tensor([2], dtype=torch.int32, device=dev())
    out = torch.zeros((H, rows, 128), dtype=dtype, device=dev())
    ops.attn_fwd(f8.q, f8.k, f8.v, out, head_list=heads, n_heads_dev=count, n_q=n_q, q_group_len=glen, n_kv=n_kv,
                 q_rows=torch.as_tensor(q_rows, device=dev()), kv_rows=torch.as_tensor(kv_rows, device=dev()),
                 kv_rows_stride_g=n_kv, dup_rows=torch.as_tensor(dup, device=dev()), n_dup_pos=60,
                 block_rows=block_rows, v_descale=f8.v_descale)
    torch.cuda.synchronize()
    q8, k8, v8, vd = _decoded(f8)
    ref, amb = np.zeros((H, rows, 128)), np.zeros((H, rows))
    for h in (3, 0):
        O.fp8_attn_launch(q8[h], k8[h], v8[h], ref[h], vd[h], n_q=n_q, n_kv=n_kv, q_rows=q_rows, q_group_len=glen,
                          kv_rows=kv_rows, dup_rows=dup, n_dup_pos=60, ambiguous=amb[h])
    _check(out, ref, dtype, amb, _vmax(v8, vd))
    assert torch.all(out[2] == 0) and torch.all(out[1] == 0)


@pytest.mark.parametrize("n_splits", [3, 8])
def test_fp8_split_keys(n_splits):
    from vorta_amd import ops
    dtype = torch.float16
    rng = np.random.default_rng(4)
    H, Sq, Skv = 2, 40, 3000
    x = [rng.standard_normal((H, Skv, 128)) for _ in range(3)]
    f8 = ops.fp8_quantize_qkv(*(to_dev(a, dtype) for a in x))
    out = torch.empty((H, Skv, 128), dtype=dtype, device=dev())
    ops.attn_fwd(f8.q, f8.k, f8.v, out, n_q=Sq, q_row_offset=100, q_valid=33, n_kv=2900, n_splits=n_splits,
                 v_descale=f8.v_descale)
    q8, k8, v8, vd = _decoded(f8)
    ref, amb = np.zeros((H, Skv, 128)), np.zeros((H, Skv))
    for h in range(H):
        O.fp8_attn_launch(q8[h], k8[h], v8[h], ref[h], vd[h], n_q=Sq, q_row_offset=100, q_valid=33, n_kv=2900,
                          n_splits=n_splits, ambiguous=amb[h])
    _check(out[:, 100:140], ref[:, 100:140], dtype, amb[:, 100:140], _vmax(v8, vd))
    assert torch.all(out[:, 133:140] == 0)


def _emulate_routed(q16, k16, v16, f8, experts, geom, model, T, te, scale=None):
    """the launches of vorta_amd/routed.py, one by one, through the oracle's emulator (tables from the GPU: they are
    pinned against the oracle by tests/test_hip_experts.py)"""
    from vorta_amd import ops
    from vorta_amd.routed import _auto_splits
    q8, k8, v8, vd = _decoded(f8)
    H, N, _ = q8.shape
    S = geom.S
    out, amb = np.zeros((H, N, 128)), np.zeros((H, N))
    hs = [[h for h in range(H) if experts[h] == e] for e in range(3)]
    for h in hs[0]:
        O.fp8_attn_launch(q8[h], k8[h], v8[h], out[h], vd[h], n_q=S + T, n_kv=S + te, q_valid=S + te, ambiguous=amb[h])
    if hs[1]:
        hl = torch.tensor(hs[1], dtype=torch.int32, device=dev())
        keep_q, drop_q = ops.coreset_select(q16, geom.latent, geom.group, geom.n_keep, tail_first=S, n_tail=T, head_list=hl)
        if model == "hunyuan":
            keep_k, _ = ops.coreset_select(k16, geom.latent, geom.group, geom.n_keep, tail_first=S, n_tail=te,
                                           head_list=hl, want_drop=False)
        else:
            keep_k = keep_q
        kq, kk, dq = keep_q.cpu().numpy(), keep_k.cpu().numpy(), drop_q.cpu().numpy()
        for y, h in enumerate(hs[1]):
            O.fp8_attn_launch(q8[h], k8[h], v8[h], out[h], vd[h], n_q=geom.S_low + T, n_kv=geom.S_low + te,
                              q_valid=geom.S_low + te, q_rows=kq[y], kv_rows=kk[y], dup_rows=dq[y], n_dup_pos=geom.G,
                              ambiguous=amb[h])
    if hs[2]:
        q_rows, kv_rows, n_kv, table, n_lists = geom.sta_launch_tables(te, 256)  # query tiles of equal key lists merged
        qr, kr, tb = q_rows.cpu().numpy(), kv_rows.cpu().numpy(), table.cpu().numpy()
        bounds = [(int(tb[tb[:, 0] == g, 1].min()), int(tb[tb[:, 0] == g, 2].max())) for g in range(n_lists)]
        assert bounds[0][0] == 0 and bounds[-1][1] == S and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
        for h in hs[2]:
            O.fp8_attn_launch(q8[h], k8[h], v8[h], out[h], vd[h], n_q=S, n_kv=n_kv, q_rows=qr, kv_rows=kr,
                              q_group_bounds=bounds, ambiguous=amb[h])
            if T:
                O.fp8_attn_launch(q8[h], k8[h], v8[h], out[h], vd[h], n_q=T, q_row_offset=S, q_valid=te, n_kv=S + te,
                                  n_splits=_auto_splits(len(hs[2]), T, S + te), ambiguous=amb[h])
    return out, amb, _vmax(v8, vd)


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("fused", [True, False])
def test_fp8_routed_attention_vs_emulator_and_oracle(model, fused):
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention
    dtype = torch.bfloat16
    latent, tile, window, group = (9, 12, 16), (3, 6, 8), (3, 3, 3), (3, 3, 2)
    H, T, te = 6, (64 if model == "hunyuan" else 0), (40 if model == "hunyuan" else 0)
    S = latent[0] * latent[1] * latent[2]
    rng = np.random.default_rng(5)
    q, k, v = (rng.standard_normal((1, H, S + T, 128)) for _ in range(3))
    experts = [0, 1, 2, 2, 1, 0]
    geom = RoutedGeometry(latent, tile, window, group, 0.5, dev())
    qd, kd, vd = to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype)
    from vorta_amd import ops
    f8 = ops.fp8_quantize_qkv(qd[0], kd[0], vd[0])
    out = routed_attention(qd, kd, vd, HeadRouting.from_expert_ids(experts, dev()), geom, model=model, text_len=T,
                           text_valid=te, fp8=True, fused=fused, fp8_operands=f8)
    torch.cuda.synchronize()
    ref, amb, vmax = _emulate_routed(qd[0], kd[0], vd[0], f8, experts, geom, model, T, te)
    _check(out[0], ref, dtype, amb, vmax)
    if T:
        assert not _bits(out[0, :, S + te:]).any()
    # against the golden-pinned fp64 oracle on the 16-bit inputs: the whole cost of the e4m3 path
    gi = O.group_info(latent, group, 0.5)
    full = O.routed_attention(rounded(q, dtype), rounded(k, dtype), rounded(v, dtype), np.array(experts), model=model,
                              latent=latent, tile=tile, window=window, gi=gi, t_text=T, t_eff=te)[0]
    o = out[0].float().cpu().numpy()
    rfs = [rel_fro(o[h], full[h]) for h in range(H)]
    print("fp8 routed vs the fp64 oracle on the 16-bit inputs, rel. Frobenius per head:", [round(x, 4) for x in rfs], experts)
    for h in range(H):
        assert rfs[h] < 0.12, (h, experts[h], rfs[h])
    # same routing through device-resident head lists
    from vorta_amd import ops as _ops
    sc = torch.zeros((1, H, 3), device=dev())
    for h, e in enumerate(experts):
        sc[0, h, e] = 1.0
    _, lists, counts = _ops.route_scores(sc, 0.3)
    out2 = routed_attention(qd, kd, vd, HeadRouting.from_device(lists, counts), geom, model=model, text_len=T,
                            text_valid=te, fp8=True, fused=fused)
    assert torch.equal(out2, out)


def test_fp8_operator_psnr_wan14b_81f_geometry():
    """gate (ii): every expert at BASELINE configs[4]'s geometry (Wan-2.1 14B 81x720x1280: S = 75 600, tile (7,9,8),
    coreset window (3,3,2)), fp8 against the bf16 kernels on the same bf16 inputs"""
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention
    dtype = torch.bfloat16
    latent, tile, window, group = (21, 45, 80), (7, 9, 8), (3, 3, 3), (3, 3, 2)
    S = latent[0] * latent[1] * latent[2]
    H = 3
    gen = torch.Generator(device=dev()).manual_seed(1234)
    q, k, v = (torch.randn((1, H, S, 128), generator=gen, device=dev(), dtype=dtype) for _ in range(3))
    geom = RoutedGeometry(latent, tile, window, group, 0.5, dev())
    routing = HeadRouting.from_expert_ids([0, 1, 2], dev())
    ref = routed_attention(q, k, v, routing, geom, model="wan")
    out = routed_attention(q, k, v, routing, geom, model="wan", fp8=True)
    torch.cuda.synchronize()
    names = ["full", "coreset", "sliding-tile"]
    table = {names[h]: _psnr(out[0, h], ref[0, h]) for h in range(H)}
    print("fp8 vs bf16 operator, Wan-14B-81f geometry (PSNR over data range dB, PSNR over max|x| dB, rel. rms error):",
          {n: tuple(round(x, 4) for x in p) for n, p in table.items()})
    assert not torch.isnan(out).any()
    for n, (p_range, p_peak, rel) in table.items():
        assert p_range >= 40.0 and p_peak >= 39.0 and rel <= 0.06, (n, p_range, p_peak, rel)


# Gates of the structured-input families (tests/_fp8_inputs.py), dB of PSNR over max|x| of the 16-bit result -- the stricter
# of the two conventions -- per expert, measured at both geometries (profiles/r03_fp8_structured_inputs.txt) and held 1 dB
# under the worst of them.  What e4m3 operands can and cannot do: a score is a sum of 128 products whose rounding errors
# (2^-4 relative at most, 2.6 % rms, for each e4m3 operand) add up to 3.7 % of the ROOT SUM OF SQUARES of the products, so
# the absolute error of a logit grows with the logits themselves.  Flat softmax (white noise, smooth fields, heavy tails,
# common components -- the key centring removes the k side, the q side is a per-key constant times a small error):
# 39-41 dB and up.  Peaked softmax (logit spread x 4): 36-38 dB.  Outlier channels from norm weights (6 channels carry the logits):
# 29-32 dB, 21-26 dB with a common part on top -- and per-channel smoothing of q and k, exact for the scores, changes
# nothing (a floating-point format keeps its relative error under any rescaling): an 8-bit path that holds 40 dB there
# needs more mantissa in q k^T, not other scales.
FAMILY_GATES = {"white": 39.0, "common3": 38.0, "student_t3": 42.0, "smooth": 55.0, "peaked": 34.5, "outlier_w": 27.5,
                "outlier_w_common": 18.5}


@pytest.mark.parametrize("geometry", ["wan14b-81f", "hunyuan-129f"])
def test_fp8_operator_psnr_on_structured_inputs(geometry):
    """gate (ii) beyond white noise, at BASELINE configs[4]'s geometry and at the headline's (with text rows): every expert,
    fp8 against the bf16 kernels on the same bf16 inputs, both PSNR conventions printed, the stricter one gated."""
    from _fp8_inputs import NAMES, families, psnr, robust_psnr, smoothed
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention
    dtype = torch.bfloat16
    if geometry == "wan14b-81f":
        latent, tile, window, group, model, T, te = (21, 45, 80), (7, 9, 8), (3, 3, 3), (3, 3, 2), "wan", 0, 0
    else:
        latent, tile, window, group, model, T, te = (33, 45, 80), (11, 9, 8), (3, 3, 3), (3, 3, 2), "hunyuan", 256, 96
    S = latent[0] * latent[1] * latent[2]
    geom = RoutedGeometry(latent, tile, window, group, 0.5, dev())
    routing = HeadRouting.from_expert_ids([0, 1, 2], dev())
    gen = torch.Generator(device=dev()).manual_seed(1234)
    kw = dict(model=model, text_len=T, text_valid=te)
    experts = ["full", "coreset", "sliding"]
    for key, q, k, v in families(latent, 3, T, gen, dev()):
        q16, k16, v16 = (x.to(dtype)[None].contiguous() for x in (q, k, v))
        ref = routed_attention(q16, k16, v16, routing, geom, **kw)
        out = routed_attention(q16, k16, v16, routing, geom, fp8=True, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all(), key
        table = {experts[h]: psnr(out[0, h, :S + te], ref[0, h, :S + te]) for h in range(3)}
        rob = {experts[h]: robust_psnr(out[0, h, :S + te], ref[0, h, :S + te]) for h in range(3)}
        # (the all-e4m3 path is gated on PSNR only: its scores carry 3 mantissa bits and its probabilities one exponent range per
        # row -- the relative error and the PSNR over the 99.9th percentile are printed for the record; "fp8pv" and "i8pv" hold
        # 0.08 relative, tests/test_hip_mx.py and tests/test_hip_i8.py)
        print(f"fp8 vs bf16 [{geometry}] {NAMES[key]}: " + ", ".join(f"{n} {a:.1f} / {b:.1f} / p99.9 {rob[n]:.1f} dB rel {c:.3f}" for n, (a, b, c) in table.items()))
        for n, (p_range, p_peak, rel) in table.items():
            assert p_peak >= FAMILY_GATES[key] and p_range >= p_peak, (geometry, key, n, p_range, p_peak, rel)
        if key == "outlier_w":  # per-channel smoothing of q, k: exact for the scores, no help for a floating-point format
            qs, ks = (x.to(dtype)[None].contiguous() for x in smoothed(q, k))
            ref2 = routed_attention(qs, ks, v16, routing, geom, **kw)
            out2 = routed_attention(qs, ks, v16, routing, geom, fp8=True, **kw)
            for h in (0, 2):  # (the coreset ranking itself changes under the rescaling: not comparable)
                gain = psnr(out2[0, h, :S + te], ref2[0, h, :S + te])[1] - table[experts[h]][1]
                assert abs(gain) < 2.5, (geometry, experts[h], gain)


@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("T", [0, 96])
def test_quantizer_sequence_shards_write_the_bytes_of_one_call(P, T):
    """The send side of the exchange converts q and k shard by shard (include/vorta_hip.h flags bit3 / bit4): every rank
    adds the sample partials of its tokens to a table (here: P calls into one zeroed table = the SUM all-reduce of P
    tables with disjoint slots), then converts its shard with the scales of the whole sequence, heads in destination
    order.  The bytes are those of ONE plain call over the assembled (H, S + T, D) sequence, bit for bit."""
    from vorta_amd import ops
    dtype = torch.bfloat16
    H, S = 5, 8 * 520  # shards of S / P tokens hold whole eighths of the video tokens
    gen = torch.Generator(device=dev()).manual_seed(11 + P + T)
    q, k, v = (torch.randn((H, S + T, 128), generator=gen, device=dev()).to(dtype) for _ in range(3))
    k = (k.float() + 2.0 * torch.randn((H, 1, 128), generator=gen, device=dev())).to(dtype)  # a centre worth subtracting
    whole = ops.fp8_quantize_qkv(q, k, v, center_k=True, video_tokens=S)
    order = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int32, device=dev())
    Sl = S // P
    nws = whole.ws.numel()
    ws = torch.full((nws,), 7.0, dtype=torch.float32, device=dev())  # stale contents everywhere but the zeroed partials
    part = ops.fp8_ws_partials(ws, H)
    part.zero_()
    dummy = torch.empty((H, 1, 128), dtype=torch.uint8, device=dev())
    shards = [(q[:, r * Sl:(r + 1) * Sl], k[:, r * Sl:(r + 1) * Sl]) for r in range(P)]
    for r, (qs, ks) in enumerate(shards):
        ops.fp8_quantize_qkv(qs, ks, None, out=ops.Fp8Operands(dummy, dummy, dummy, whole.v_descale, ws), center_k=True,
                             phase="stats", token_offset=r * Sl, total_tokens=S + T, video_tokens=S)
    if T:
        ops.fp8_quantize_qkv(q[:, S:], k[:, S:], None, out=ops.Fp8Operands(dummy, dummy, dummy, whole.v_descale, ws),
                             center_k=True, phase="stats", token_offset=S, total_tokens=S + T, video_tokens=S)
    assert torch.equal(part, ops.fp8_ws_partials(whole.ws, H))  # the partial tables agree slot for slot
    q8 = torch.zeros((H, S + T, 128), dtype=torch.uint8, device=dev())
    k8 = torch.zeros_like(q8)
    pieces = [(qs, ks, r * Sl, slice(r * Sl, (r + 1) * Sl)) for r, (qs, ks) in enumerate(shards)]
    if T:
        pieces.append((q[:, S:], k[:, S:], S, slice(S, S + T)))
    for qs, ks, off, sl in pieces:
        ops.fp8_quantize_qkv(qs, ks, None, out=ops.Fp8Operands(q8[:, sl], k8[:, sl], dummy, whole.v_descale, ws),
                             center_k=True, phase="convert", token_offset=off, total_tokens=S + T, video_tokens=S,
                             src_map=order)
    torch.cuda.synchronize()
    o = order.long()
    assert torch.equal(q8, whole.q[o]) and torch.equal(k8, whole.k[o])
    # a negative map entry leaves that output head alone (a rank writes the text rows of ITS heads only)
    part_map = torch.tensor([3, -1, 4, -1, -1], dtype=torch.int32, device=dev())
    q8b = torch.full((H, Sl, 128), 77, dtype=torch.uint8, device=dev())
    k8b = torch.full_like(q8b, 77)
    ops.fp8_quantize_qkv(shards[0][0], shards[0][1], None, out=ops.Fp8Operands(q8b, k8b, dummy, whole.v_descale, ws),
                         center_k=True, phase="convert", token_offset=0, total_tokens=S + T, video_tokens=S, src_map=part_map)
    assert torch.equal(q8b[0], whole.q[3, :Sl]) and torch.equal(k8b[2], whole.k[4, :Sl])
    assert (q8b[[1, 3, 4]] == 77).all() and (k8b[[1, 3, 4]] == 77).all()
    # a statistics call whose shard cuts a sample chunk is refused (nobody would sum that chunk: empty sample, no error)
    for off, n in ((0, Sl - 8), (8, Sl - 8), (S // 8 + 16, S // 8)):
        with pytest.raises(ValueError):  # VORTA_EINVAL
            ops.fp8_quantize_qkv(q[:, off:off + n], k[:, off:off + n], None,
                                 out=ops.Fp8Operands(dummy, dummy, dummy, whole.v_descale, ws), center_k=True, phase="stats",
                                 token_offset=off, total_tokens=S + T, video_tokens=S)
