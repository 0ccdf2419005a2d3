"""The yardstick of the structured-input forward tests: a ROUNDING MODEL of the 16-bit attention forward, the input
families and launches it is measured on, and a float32 EMULATION of the kernel's loop that shows the tests' bounds can be
met (tests/test_host_forward_model.py, tests/test_hip_attention_fwd_structured.py).

`model_out` is the float64 forward of one launch dictionary, walked with the geometry of tests/_attn_restate.py, with exactly
the three roundings to 16 bits that the kernels of csrc/attn_fwd.hip make by design:

    Qs  = round16(q scale log2 e)                 attn_fwd.hip:348   qf[ks][i] = (T)((float)raw[i] * p.scale_log2);
          (the pipelined kernel only; variant 1, the plain kernel of lines 27-279, multiplies in float32 -- line 187,
           exp2f(fmaf(s0[i], c, -mc)) -- and does not round)
    P16 = round16(exp2(z - max_j z))              attn_fwd.hip:600-603 / 194-197   pb_[0][e_] = (T)c0_[e_];
          feeds the P V product; the row sum l is taken from the unrounded P
                                                  attn_fwd.hip:593-598 / 186-191   lsum_ += c0_[i_] + c1_[i_];
    out = round16(P16 V / l)                      attn_fwd.hip:741 / 259           t[j] = (T)(o[dt][4 * rg + j] * inv);

zeros at positions >= the effective q_valid, duplicate rows copied.  With round16=False it is plain float64 attention, which
tests/test_host_forward_model.py pins against the restatement.

The kernel rounds P relative to a reference point that lags the row maximum by up to 2^6 (defer_log2, attn_fwd.hip:586),
the model relative to the maximum: a non-integer offset changes which way single values round, so kernel and model agree
statistically, not bit by bit, and the tests compare ERRORS against float64, not outputs.

`emulate_out` is the loop itself in float32 torch: Qs rounded, 64-key blocks, the reference point fixed by the first block
and raised only when a row of the wave (32 positions) is more than 6 above it, P rounded, l from the float32 P, splits merged
as attn_combine_kernel merges them.  It is what the margins of the tests' bounds are measured against -- the kernel never
is -- and what the mutations of tests/test_host_forward_model.py are applied to.

Nothing here reads the library."""
import functools
import math

import numpy as np
import torch

import _attn_bwd_model as M
import _random_launch as RL
from _attn_bwd_model import _cpu, _walk, dtype_name, fro  # noqa: F401
from _attn_restate import launch_geometry

LOG2E = 1.4426950408889634
KVB = 64  # keys per block of the loop
DEFER = 6.0  # attn_fwd.hip:841
DTYPES = M.DTYPES
FAMILIES = ("white", "local", "redundant", "shift_up", "shift_down", "late_key", "staircase", "v_common")
S_VID = M.S_VID
STAIR_RISE = 4.0  # log2 units per 64-key block
STAIR_Q = 4.0  # the queries' component along the staircase direction


# ----------------------------------------------------------------------------------------------------------- the inputs
def family(name, H, S, dtype, seed=7):
    """(q, k, v) of one input family as (H,S,128) CPU tensors rounded to `dtype`; six are tests/_attn_bwd_model.py's.
    staircase: q = w + 4 u, k_j = w_j + b_j u with the white parts orthogonal to the unit vector u and b_j growing linearly
    along the sequence, so that the score of key j carries 4 j / 64 log2 units on top of its noise: the row maximum rises by
    about 4 per 64-key block of a contiguous key range (|k_j| grows from 11 to about 50 over 400 keys).
    v_common: v + 4, the output is a common part plus little, so the final rounding is the error"""
    assert name in FAMILIES
    if name not in ("staircase", "v_common"):
        return M.family(name, H, S, dtype, seed)[:3]
    q, k, v, _ = (x.float() for x in M.family("white", H, S, dtype, seed))
    if name == "v_common":
        return q.to(dtype), k.to(dtype), (v + 4).to(dtype)
    gen = torch.Generator(device="cpu").manual_seed(seed + 1)
    u = torch.randn(128, generator=gen)
    u = u / u.norm()
    q, k = q - (q @ u)[..., None] * u, k - (k @ u)[..., None] * u
    c = LOG2E / math.sqrt(128)
    b = torch.arange(S, dtype=torch.float32) * (STAIR_RISE / KVB / (STAIR_Q * c))
    return (q + STAIR_Q * u).to(dtype), (k + b[None, :, None] * u).to(dtype), v.to(dtype)


# ----------------------------------------------------------------------------------------------------------- the launches
# name -> (H, S, keywords, variant).  Which path of the pipelined loop (attn_fwd.hip:659-676: blk_whole = whole blocks - 2,
# or - 3 with a key table; the main loop runs PAIRS of steps below it, the tail steps take the rest) a key count reaches:
#   n_kv  64  one block: the prologue, then one tail step that ends the pair early (line 674)
#   n_kv  65  two blocks, the second of one key: two tail steps, the mask of the partial block
#   n_kv 128  two whole blocks: blk_whole = 0, two tail steps and no mask
#   n_kv 192  three blocks: blk_whole = 1, no main-loop pair, three tail steps (an odd count: the early break again)
#   n_kv 321  five blocks and one key: blk_whole = 3, one main-loop pair, the rows rebuilt (lines 665-671), four tail steps
#   n_kv 371  (dense_tail) the same with a wider partial block and row offsets
#   n_kv 384  (dense) six whole blocks: two main-loop pairs, two tail steps
#   dense, 3 splits: two blocks per split, blk_whole = min(blk1, 4): split 0 runs its two blocks in the main loop, splits 1 and 2 in tail steps
#   dense, 8 splits: one block per split, splits 6 and 7 are empty (m = -1e30, l = 0 into the merge)
#   fused_table: a key table of 460 keys, 7 blocks and 12 keys: blk_whole = 4, two main-loop pairs with row-id loads, four
#                tail steps (gather_a's 228 keys have blk_whole = 0: tail steps only)
# The gather launches are tests/_attn_bwd_model.py's seeds.  Both carry n_splits = 1; seed 24 (gather_a) block_rows = 128
# with its q_block_table, seed 9 (gather_b) block_rows = 0, which the library resolves to 128 rows for one group of 268
# queries.  So `n_splits=1` forced through RL.kwargs is what they already run (gather_*_s1 pins that: the same launch), and
# the forced n_splits = 3 is what takes them through the split path (gather_a: 4 blocks, 2 per split, the third empty).
_FUSED_S = 480


def _fused_tables():
    rng = np.random.default_rng(77)
    return (rng.permutation(_FUSED_S)[:460].astype(np.int32), rng.permutation(_FUSED_S)[:300].astype(np.int32))


def _gather(name, **over):
    L = RL.draw(np.random.default_rng(M.GATHER_SEEDS[name]), H_buf=2, S=400)
    return (L.H_buf, L.S, lambda dev: RL.kwargs(L, dev, **over))


_DENSE = dict(n_q=S_VID, n_kv=S_VID)
_TAIL = dict(n_q=340, q_row_offset=37, q_valid=300, n_kv=371, kv_row_offset=19)
_LAUNCHES = {
    "dense_128": (1, S_VID, lambda dev: dict(_DENSE, block_rows=128), 0),
    "dense_256": (1, S_VID, lambda dev: dict(_DENSE, block_rows=256), 0),
    "dense_tail": (1, 400, lambda dev: dict(_TAIL), 0),
    "gather_a": _gather("gather_a") + (0,),
    "gather_b": _gather("gather_b") + (0,),
    "gather_a_s1": _gather("gather_a", n_splits=1) + (0,),
    "gather_b_s1": _gather("gather_b", n_splits=1) + (0,),
    "gather_a_s3": _gather("gather_a", n_splits=3) + (0,),
    "gather_b_s3": _gather("gather_b", n_splits=3) + (0,),
    "dense_s3": (1, S_VID, lambda dev: dict(_DENSE, n_splits=3), 0),
    "dense_s8": (1, S_VID, lambda dev: dict(_DENSE, n_splits=8), 0),
    "dense_tail_v1": (1, 400, lambda dev: dict(_TAIL, variant=1), 1),
    "gather_b_v1": _gather("gather_b", variant=1) + (1,),
    # q_valid inside a wave (positions 288 .. 319): the rows past it are written as zeros whatever their q rows hold
    "dense_qvalid": (1, S_VID, lambda dev: dict(_DENSE, q_valid=300), 0),
    "dense_qvalid_v1": (1, S_VID, lambda dev: dict(_DENSE, q_valid=300, variant=1), 1),
    "dense_strided": (3, S_VID, lambda dev: dict(_DENSE), 0),  # the GPU test passes (S, H, D) storage views
    # one fused grid of three 256-row launches over one (2, 480, 128) operand set
    "fused_dense": (2, _FUSED_S, lambda dev: dict(n_q=420, q_row_offset=11, n_kv=_FUSED_S, block_rows=256), 0),
    "fused_table": (2, _FUSED_S, lambda dev: dict(n_q=300, q_rows=torch.as_tensor(_fused_tables()[1], device=dev), n_kv=460,
                                                  kv_rows=torch.as_tensor(_fused_tables()[0], device=dev), q_valid=290,
                                                  block_rows=256), 0),
    "fused_splits": (2, _FUSED_S, lambda dev: dict(n_q=256, q_row_offset=200, n_kv=450, kv_row_offset=30, n_splits=3,
                                                   block_rows=256), 0),
}
KV_COUNTS = (64, 65, 128, 192, 321)
for _n in KV_COUNTS:
    _LAUNCHES[f"kv{_n}"] = (1, S_VID, lambda dev, n=_n: dict(n_q=S_VID, n_kv=n), 0)
FUSED = ("fused_dense", "fused_table", "fused_splits")
LAUNCHES = tuple(n for n in _LAUNCHES if not n.startswith("kv"))
CASES = tuple((f, w) for f in FAMILIES for w in LAUNCHES) + tuple((f, f"kv{n}") for f in ("white", "late_key") for n in KV_COUNTS)


def launch(name, device="cpu"):
    """(H, S, launch keywords with their tables on `device`, variant) of one launch"""
    H, S, kw, variant = _LAUNCHES[name]
    return H, S, kw(device), variant


# ------------------------------------------------------------------------------------------------------------- the model
def model_out(kw, q, k, v, dtype, round16=True, variant=0, work=torch.float64, fill=0.0):
    """(H,S,D) output of one launch (rows it does not write hold `fill`), computed in `work` (float64: the model; float32
    with round16=False: a plain float32 forward), returned in float64.  q, k, v: (H,S,D) of any dtype"""
    r16 = (lambda x: x.to(dtype).to(work)) if round16 else (lambda x: x)
    q, k, v = (x.detach().cpu().to(work) for x in (q, k, v))
    H = q.shape[0]
    q_valid = launch_geometry(kw, H)[3]
    c = (kw.get("scale") or 1.0 / math.sqrt(q.shape[-1])) * LOG2E
    dup = _cpu(kw.get("dup_rows"))
    out = torch.full(q.shape, fill, dtype=work)
    for y, h, qr, segs in _walk(kw, H):
        for a, b, keys in segs:
            rows, K, V = qr[a:b], k[h, keys], v[h, keys]
            z = r16(q[h, rows] * c) @ K.t() if variant != 1 else (q[h, rows] @ K.t()) * c
            P = torch.exp2(z - z.max(-1, keepdim=True).values)
            o = r16((r16(P) @ V) / P.sum(-1, keepdim=True))
            o[torch.arange(a, b) >= q_valid] = 0
            out[h, rows] = o
        if dup is not None:
            dr = dup[y] if dup.dim() == 3 else dup
            npos = kw.get("n_dup_pos", 0) or dr.shape[0]
            for i in range(dr.shape[1]):
                out[h, dr[:npos, i]] = out[h, qr[:npos]]
    return out.double()


def row_masks(kw, shape):
    """boolean (H,S) masks of one launch: (rows at positions below the effective q_valid, rows at positions past it, rows
    that are duplicates) -- every other row is not written"""
    valid, zero, dups = (torch.zeros(shape[:2], dtype=torch.bool) for _ in range(3))
    q_valid = launch_geometry(kw, shape[0])[3]
    dup = _cpu(kw.get("dup_rows"))
    for y, h, qr, segs in _walk(kw, shape[0]):
        for a, b, _ in segs:
            valid[h, qr[a:min(b, q_valid)]] = True
            zero[h, qr[max(a, q_valid):b]] = True
        if dup is not None:
            dr = dup[y] if dup.dim() == 3 else dup
            dups[h, dr[: kw.get("n_dup_pos", 0) or dr.shape[0]].reshape(-1)] = True
    return valid, zero, dups


def dup_pairs(kw, H):
    """[(head, duplicate rows, their source rows)] of one launch"""
    dup = _cpu(kw.get("dup_rows"))
    pairs = []
    if dup is not None:
        for y, h, qr, _ in _walk(kw, H):
            dr = dup[y] if dup.dim() == 3 else dup
            npos = kw.get("n_dup_pos", 0) or dr.shape[0]
            pairs += [(h, dr[:npos, i], qr[:npos]) for i in range(dr.shape[1])]
    return pairs


# --------------------------------------------------------------------------------------------------------- the emulation
# Sums and exp2 are taken in float64 and rounded to float32 once (a float32 result that does not depend on the order of a
# BLAS or on a vector exp of the host); products, scalings and running sums are single float32 operations
def _mm(a, b):
    return (a.double() @ b.double()).float()


def _exp2(x):
    return torch.exp2(x.double()).float()


def _emulate_split(z, V, n_keys, blk0, blk1, dtype, variant, c32, wave0, info):
    """one key split of one query segment: z (rows, keys) float32 scores -- variant 0: in the exp2 domain; variant 1: raw,
    scaled by c32 inside the exponent as line 187 does -- of ALL keys; returns (o, m in the exp2 domain, l)"""
    n = z.shape[0]
    o, l = torch.zeros((n, V.shape[1])), torch.zeros(n)
    m = torch.full((n,), -1e30)
    wave = (torch.arange(n) + wave0) // 32  # the rows that share a wave: 32 positions from the start of the group
    for blk in range(blk0, blk1):
        zb, Vb = z[:, blk * KVB: min((blk + 1) * KVB, n_keys)], V[blk * KVB: min((blk + 1) * KVB, n_keys)]
        mx = zb.max(-1).values
        if variant == 1:  # the exact running maximum, rescaled whenever it moves (lines 173-182)
            m_new = torch.maximum(m, mx)
            alpha = _exp2((m - m_new) * c32)
            o, l, m = o * alpha[:, None], l * alpha, m_new
            P = _exp2(zb * c32 - (m * c32)[:, None])
        else:
            if blk == blk0:
                m = mx.clone()  # the first block fixes the reference point at its row maximum (line 647)
            else:
                over = mx - m
                raise_ = torch.zeros(n, dtype=torch.bool)
                for w in wave.unique():  # !__all(mx_cur <= defer): the whole wave moves, each row by max(mx_cur, 0)
                    if (over[wave == w] > DEFER).any():
                        raise_ |= wave == w
                g = torch.where(raise_, over.clamp(min=0), torch.zeros(n))
                if info is not None:
                    info["raises"] = info.get("raises", 0) + int((g > 0).sum())
                    info["max_lag"] = max(info.get("max_lag", 0.0), float((over - g).max()))
                alpha = _exp2(-g)
                o, l, m = o * alpha[:, None], l * alpha, m + g
            P = _exp2(zb - m[:, None])
        l = l + P.double().sum(-1).float()
        o = o + _mm(P.to(dtype), Vb)
    return o, (m * c32 if variant == 1 else m), l


def emulate_out(kw, q, k, v, dtype, variant=0, fill=0.0, mutate=None, info=None):
    """(H,S,D) float64 output of the float32 emulation of one launch.  `mutate`, a wrong kernel for the tests of the gates:
    ("drop_key", head, position, key index) masks one key of one row; ("scale_channel", channel, factor) scales one output
    channel before the final rounding; ("shift_kv", group) reads every key row of one group one row further"""
    q, k, v = (x.detach().cpu().float() for x in (q, k, v))
    H, S = q.shape[:2]
    _, _, n_kv, q_valid = launch_geometry(kw, H)
    c32 = float(np.float32(kw.get("scale") or 1.0 / math.sqrt(q.shape[-1])) * np.float32(LOG2E))
    n_splits = kw.get("n_splits", 1)
    bps = -(-(-(-kw["n_kv"] // KVB)) // n_splits)  # blocks per split, cut from the HOST n_kv (attn_fwd.hip:859-860)
    nblk = -(-n_kv // KVB)
    dup = _cpu(kw.get("dup_rows"))
    out = torch.full(q.shape, fill, dtype=torch.float64)
    for y, h, qr, segs in _walk(kw, H):
        for gi, (a, b, keys) in enumerate(segs):
            if mutate and mutate[0] == "shift_kv" and mutate[1] == gi:
                keys = (keys + 1) % S
            rows, K, V = qr[a:b], k[h, keys], v[h, keys]
            Q = q[h, rows]
            z = _mm((Q * c32).to(dtype), K.t()) if variant != 1 else _mm(Q, K.t())
            if mutate and mutate[0] == "drop_key" and mutate[1] == h and a <= mutate[2] < b:
                z[mutate[2] - a, mutate[3]] = -float("inf")
            parts = [_emulate_split(z, V, n_kv, min(s * bps, nblk), min(s * bps + bps, nblk), dtype, variant, c32, 0, info)
                     for s in range(n_splits)]
            if n_splits == 1:
                o, _, l = parts[0]
            else:  # attn_combine_kernel (attn_common.h:118-128)
                m = torch.stack([p[1] for p in parts]).max(0).values
                o, l = torch.zeros_like(parts[0][0]), torch.zeros_like(m)
                for po, pm, pl in parts:
                    w = _exp2(pm - m)
                    l = l + w * pl
                    o = o + w[:, None] * po
            o = o * (1.0 / l)[:, None]
            if mutate and mutate[0] == "scale_channel":
                o[:, mutate[1]] *= mutate[2]
            o = o.to(dtype).double()
            o[torch.arange(a, b) >= q_valid] = 0
            out[h, rows] = o
        if dup is not None:
            dr = dup[y] if dup.dim() == 3 else dup
            npos = kw.get("n_dup_pos", 0) or dr.shape[0]
            for i in range(dr.shape[1]):
                out[h, dr[:npos, i]] = out[h, qr[:npos]]
    return out


# ----------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def case(fam, dtype, which):
    """everything the tests need of one (family, dtype, launch), computed once on the CPU and left unchanged: the inputs, the
    float64 output, the model's, a plain float32 one, the emulation's, and the row masks"""
    H, S, kw, variant = launch(which)
    q, k, v = family(fam, H, S, dtype)
    f64 = model_out(kw, q, k, v, dtype, round16=False)
    model = model_out(kw, q, k, v, dtype, variant=variant)
    f32 = model_out(kw, q, k, v, dtype, round16=False, work=torch.float32)
    emu = emulate_out(kw, q, k, v, dtype, variant=variant)
    valid, zero, dups = row_masks(kw, (H, S))
    return dict(H=H, S=S, kw=kw, variant=variant, q=q, k=k, v=v, f64=f64, model=model, f32=f32, emu=emu, valid=valid,
                zero=zero, dups=dups)


# ------------------------------------------------------------------------------------------------------------- the rule
C_ROW = 3.0  # the smallest of {3, 4} at which the emulation stays at or under MARGIN of the bound on every row of every case
C_CH = 3.0  # the same for the channels (tests/test_host_forward_model.py::test_the_emulation_meets_the_rule_with_margin)
MARGIN = 0.9


def unit_ratios(got, c, c_row=C_ROW, c_ch=C_CH):
    """{unit: e_got / bound} of an output against the case's references, absolute 2-norms against float64 with no division:
    "tensor" (one number, bound 2 e_model + 4 e_f32), "row" (one per written row below q_valid, c_row e_model + 4 e_f32
    over its 128 channels), "channel" (one per live head and channel over those rows, c_ch e_model + 4 e_f32)"""
    valid = c["valid"]
    d_got, d_model, d_f32 = ((x.double() - c["f64"]) * valid[..., None] for x in (got, c["model"], c["f32"]))
    n = lambda x, dim: torch.linalg.vector_norm(x, dim=dim)  # noqa: E731
    live = valid.any(1)
    tiny = 1e-300
    return {
        "tensor": n(d_got, None) / (2.0 * n(d_model, None) + 4.0 * n(d_f32, None)).clamp(min=tiny),
        "row": (n(d_got, 2) / (c_row * n(d_model, 2) + 4.0 * n(d_f32, 2)).clamp(min=tiny))[valid],
        "channel": (n(d_got, 1) / (c_ch * n(d_model, 1) + 4.0 * n(d_f32, 1)).clamp(min=tiny))[live],
    }
