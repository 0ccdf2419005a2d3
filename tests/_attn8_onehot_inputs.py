"""Inputs on which the three 8-bit attention forwards are exact (tests/test_hip_attention_onehot_8bit.py,
tests/test_host_attention_onehot_8bit.py): the one-hot rows of tests/_attn_onehot_inputs.py (`OH`) with e4m3 v, for

  fp8  all e4m3 (csrc/attn_fwd_fp8.hip)            q, k = the sign vectors written as the e4m3 bytes of +-A (A = 2 or 5)
  mx   16-bit scores, e4m3 P V (attn_fwd_mx.hip)   q, k = 5 x sign vectors in the 16-bit type, scale = SCALE
  i8   int8 scores, e4m3 P V (attn_fwd_i8.hip)     q as for mx; keys +-127 with hand-built operands: centre 0, balance 1,
                                                   k_bias 0, one head scale (`i8_head_scale`)

SCALE = 0.4 ln 2, not OH.SCALE: the mx kernel's q' = round16(5 scale log2 e) is then 2 and every score a multiple of 20 (the i8
head scale is chosen for the same step, to 1e-7).  The mx and i8 kernels move a wave's reference point from the maximum of
the first block of its split by WHOLE binades, so with OH.SCALE (a step of 6.37 log2 units) the chosen key's probability is a
power of two only in that first block and e4m3(2^fraction) elsewhere: still an exact row, (P v) / P, but on some rows within
the emulator's 1e-4 of a rounding midpoint (measured: 5 rows of the 16 mx launches, normalised mass 1.05), and the host test
leaves no row out.  With whole-number scores every probability is a power of two, as in the fp8 kernel.  The step is 20 and
not 10 because of the mx kernel's floor under a tile's exponent (e >= -72): after a move the scores are 8 mod the step, and
under a step of 10 a key 82 below the reference point is 2^-10 under that floor, the midpoint of the smallest e4m3 step.

    v8 = random e4m3 bytes per (head, row, channel);  v_descale (H, 128) = powers of two in 2^-2 .. 2^2 per head and channel;
    expected row of a query = e4m3_decode(v8[head, its key]) x v_descale[head]: 4 significant bits, exact in bf16 and fp16.

The bytes exclude the two NaNs (0x7F, 0xFF) and negative zero (0x80), so every byte is a distinct finite value, and zero
(0x00): the float64 launch emulator keeps, in a channel whose chosen byte is zero, the 2^-150 remainder of the blocks in
front of the chosen key (the kernels' float32 rescale factor is 0 there), and the host test compares float64 with `==`.

`best_key_gaps` measures, on the operands the kernel multiplies, the lead of the chosen key over the second best of every
wave the launch computes: the tests assert >= OH.MIN_GAP (160) log2 units before any launch.  Every other probability and
every rescale factor is then exp2(<= -155) = 0, in float32 and as an e4m3 byte.  Nothing here reads the library."""
from types import SimpleNamespace

import numpy as np
import torch

import _attn_onehot_inputs as OH
import _random_launch as RL
from oracle import vorta_oracle as O

FAMILIES = ("fp8", "mx", "i8")
DTYPES = (torch.bfloat16, torch.float16)
N_SEEDS = 16
N_GRID_SEEDS = 3
SCALE = 0.4 * float(np.log(2.0))  # (mx, i8) 5 x scale x log2 e = 2: scores in steps of 20 log2 units
STEP = 20.0
V_BYTES = np.array([b for b in range(256) if b not in (0x00, 0x7F, 0x80, 0xFF)], dtype=np.uint8)
TIE_BYTES = O.e4m3_encode(np.arange(1.0, 17.0))  # the integers 1 .. 16: no sum of tied rows is zero (see the zero byte)


# one stream of launches per family, each taken because its 16 launches reach every feature and every slip of
# tests/test_host_attention_onehot_8bit.py at least three times (asserted there at two)
STREAMS = dict(fp8=10500, mx=11200, i8=11300)


def draw(family, seed):
    return RL.draw(np.random.default_rng(STREAMS[family] + seed), S_range=(64, 600))


def plain_launch(H, S, n_q, n_kv, n_splits):
    """a launch of tests/_random_launch.py's form without tables: every head, rows 0 .. n_q - 1, keys 0 .. n_kv - 1"""
    return SimpleNamespace(H_buf=H, S=S, heads=np.arange(H, dtype=np.int32), n_heads_dev=None, block_rows=0, mode="one", glen=0,
                           bounds=[(0, n_q)], qtab=None, n_q=n_q, q_rows=None, q_off=0, kv_rows=None, kv_off=0, per_group=False,
                           n_kv=n_kv, q_valid=n_q, n_splits=n_splits, dup=None, n_dup_pos=0, n_kv_dev=None, q_valid_dev=None,
                           written=np.arange(n_q, dtype=np.int32), n_kv_eff=n_kv, q_valid_eff=n_q,
                           live=np.arange(H, dtype=np.int32))


def forced_choices(L):
    """OH.forced_choices(L) and, among the effective keys: 31 / 32 (the edge of a 32-key probability-scale group of the mx and
    i8 kernels), 127 / 128 (the first key block whose P V runs after the two-block lag), the last whole block's last key and
    the partial block's first.  The last effective key comes first: the first position of every group chooses it"""
    whole = L.n_kv_eff // OH.KVB * OH.KVB
    want = set(OH.forced_choices(L)) | {31, 32, 127, 128, whole - 1, whole}
    last = L.n_kv_eff - 1
    return [last] + sorted(c for c in want if 0 <= c < L.n_kv_eff and c != last)


def options(family, seed):
    """the fp8_opts of the launches of (family, seed); the first is the default.  Every set must write the same bits.
    (p_bias, defer) other than the default on seeds with A = 5 only: with A = 2 the scores are multiples of 8 and a key 16
    below the reference point is, under p_bias 6, the e4m3 rounding midpoint 2^-10, which the emulator counts as in doubt"""
    opts = [None]
    if family == "fp8":
        if seed % 4 == 0:
            opts.append(dict(flags=1))  # the row sum on the VALU
        if seed in (1, 9):
            opts.append(dict(p_bias=6.0, defer=2.0))
        if seed in (5, 13):
            opts.append(dict(p_bias=2.0, defer=6.0))
    elif seed % 4 == 1:
        opts.append(dict(defer=1.0))
    return opts


class Case:
    """one launch L of one family on one-hot inputs; `v8` / `vd` given: an operand set shared with other launches"""

    def __init__(self, family, L, seed, dtype, v8=None, vd=None, k=None, choice=None):
        self.family, self.L, self.seed, self.dtype = family, L, seed, dtype
        rng = np.random.default_rng(60_000 + 100 * FAMILIES.index(family) + seed)
        H, S = L.H_buf, L.S
        self.v8 = rng.choice(V_BYTES, size=(H, S, 128)) if v8 is None else v8
        self.vd = (2.0 ** rng.integers(-2, 3, size=(H, 128))).astype(np.float32) if vd is None else vd
        if k is None:  # the random launches: OH.inputs as they are, but for the longer list of forced choices
            q, k, _, choice = OH.inputs(L, seed)
            forced = forced_choices(L)
            for a, b in L.bounds:
                n = min(len(forced), b - a)
                choice[a:a + n] = forced[:n]
            for g, (a, b) in enumerate(L.bounds):
                keys = OH.key_list(L, g)
                for h in range(H):
                    q[h, L.written[a:b]] = k[h, keys[choice[a:b]]]
        else:  # the ties: q row p is the k row of choice[p]
            q = 5.0 * rng.choice([-1.0, 1.0], size=k.shape)
            q[:, L.written] = k[:, choice]
        self.choice = choice
        self.A = (2.0, 5.0)[seed % 2] if family == "fp8" else 5.0
        self.q, self.k = q * (self.A / 5.0), k * (self.A / 5.0)
        self.v_eff = expected_rows(self.v8, self.vd)
        if family == "fp8":
            self.q8, self.k8 = O.e4m3_encode(self.q), O.e4m3_encode(self.k)
            assert (O.e4m3_decode(self.q8) == self.q).all() and (O.e4m3_decode(self.k8) == self.k).all()
        else:
            # what the kernels multiply: q premultiplied by scale log2 e and re-rounded to the 16-bit type (mx); the wave's
            # int8 conversion restated by O.i8_wave_operands (i8)
            c0 = float(np.float32(SCALE) * np.float32(OH.LOG2E))
            self.qe = (torch.as_tensor(self.q).to(dtype).float() * c0).to(dtype).double().numpy()
            assert (self.qe == self.q * (STEP / 50.0)).all()
        if family == "i8":
            self.k8 = np.rint(self.k * (127.0 / 5.0)).astype(np.int8)
            self.k_bias = np.zeros((H, S), np.float32)
            self.q_prep = np.stack([np.zeros((H, 128), np.float32), np.ones((H, 128), np.float32)], 1)
            self.k_head_scale = np.full(H, i8_head_scale(), np.float32)

    def wave_operands(self, h, rows, keys):
        """(Q, K) of one wave (<= 32 query rows of head h) with Q K^T = its float64 scores in the exp2 domain"""
        if self.family == "i8":
            return O.i8_wave_operands(self.q[h][rows], self.q_prep[h], self.k_head_scale[h], self.k8[h][keys],
                                      self.k_bias[h][keys], SCALE)
        return (self.q if self.family == "fp8" else self.qe)[h][rows], self.k[h][keys]

    def emulate(self, h, out, amb, opts=None, vd=None, q_src=None, **over):
        """O.fp8_attn_launch for head h in the family's mode, writing out (S, 128) and amb (S,); `over` replaces launch
        keywords, `vd` the head's v_descale; `q_src` (S,): the query operand of row r is taken from row q_src[r]"""
        kw = dict(RL.emulator_kwargs(self.L), **over)
        o = opts or {}
        vd = self.vd[h].astype(np.float64) if vd is None else vd
        v = O.e4m3_decode(self.v8[h])
        src = np.arange(self.L.S) if q_src is None else q_src
        if self.family == "fp8":
            O.fp8_attn_launch(self.q[h][src], self.k[h], v, out, vd, ambiguous=amb, p_bias=o.get("p_bias", 5.0),
                              defer=o.get("defer", 3.0), **kw)
        elif self.family == "mx":
            O.fp8_attn_launch(self.qe[h][src], self.k[h], v, out, vd, ambiguous=amb, p_mode="rne_mx", defer=o.get("defer", 24.0),
                              **kw)
        else:
            O.fp8_attn_launch(None, None, v, out, vd, ambiguous=amb, p_mode="mx", defer=o.get("defer", 24.0),
                              wave_operands=lambda qr, kr: self.wave_operands(h, src[qr], kr), **kw)

    def expected(self, attend=OH.pick_chosen):
        """(H_buf, S, 128) float64: the chosen key's decoded v row times v_descale, zeros, duplicates, the sentinel"""
        return RL.dense_reference(self.L, self.q, self.k, self.v_eff, attend)

    def device(self, dev):
        """q, k, v, v_descale on `dev` as ops.attn_fwd takes them; for i8 also `i8` = the tensors of ops.I8Operands"""
        t = lambda a, dt=None: torch.as_tensor(a).to(dev) if dt is None else torch.as_tensor(a).to(dt).to(dev)  # noqa: E731
        d = dict(v=t(self.v8), v_descale=t(self.vd))
        if self.family == "fp8":
            d.update(q=t(self.q8), k=t(self.k8))
        elif self.family == "mx":
            d.update(q=t(self.q, self.dtype), k=t(self.k, self.dtype))
        else:
            H = self.L.H_buf
            k8 = t(self.k8)
            d.update(q=t(self.q, self.dtype), k=k8, i8=(k8, t(self.k_bias), t(self.q_prep), t(self.k_head_scale),
                                                        torch.zeros(2 * H * 128 + H, dtype=torch.float32, device=dev)))
        return d


def i8_head_scale():
    """the key scale under which one +-1 agreement of q and k moves an int8 score by STEP log2 units: the kernel's unit is
    u = (sq c0) sk in float32 with sq = 5 / 127, the query scale of a wave of +-5 rows, and a score is u 127^2 (2 a - 128)"""
    f32 = np.float32
    sq_c0 = f32(f32(5.0) * f32(1.0 / 127.0)) * f32(f32(SCALE) * f32(OH.LOG2E))
    return f32(STEP / (2.0 * 127.0 ** 2 * float(sq_c0)))


def case(family, seed):
    """the random launch of (family, seed), the dtypes alternating by seed"""
    return Case(family, draw(family, seed), seed, DTYPES[seed % 2])


def grid_cases(family, seed):
    """2 .. 6 random 256-row launches over one (H, S) set of k, v8, v_descale, drawn like `_segments` of
    tests/test_hip_attention_random.py (one in four with no live head slot); every launch has the q of its own one-hot rows.
    (odd seeds: the fp8 launches share the keys of A = 5)"""
    rng = np.random.default_rng(9700 + 100 * FAMILIES.index(family) + seed)
    dtype = DTYPES[seed % 2]
    H, S = int(rng.integers(1, 5)), int(rng.integers(200, 600))
    cases = []
    for i in range(int(rng.integers(2, 7))):
        L = RL.draw(rng, H_buf=H, S=S, block_rows=256)
        if rng.integers(0, 4) == 0:
            L.n_heads_dev, L.live = 0, L.heads[:0]
        shared = dict(v8=cases[0].v8, vd=cases[0].vd) if cases else {}
        cases.append(Case(family, L, 2 * seed + 1 + 100 * i, dtype, **shared))
    return cases


def expected_rows(v8, vd):
    """decode(v8) x v_descale per (head, row, channel) as float64; the cast to bf16 and to fp16 is exact"""
    v = O.e4m3_decode(v8) * vd[:, None, :].astype(np.float64)
    assert np.isfinite(v).all()
    for dt in DTYPES:
        assert (torch.as_tensor(v).to(dt).double().numpy() == v).all(), dt
    return v


def best_key_gaps(c, tied=None):
    """(smallest lead of the best key over the best of the others, in log2 units, over every wave the launch computes; whether the
    best key is the chosen one on every such row) from the float64 scores of the operands the kernel multiplies.
    `tied[p]`: the key positions that share position p's best score (default: its chosen key alone); they must all hold
    the maximum, and the lead is over the keys outside the set"""
    L = c.L
    worst, chosen = np.inf, True
    for h in L.live:
        for g, (a, b) in enumerate(L.bounds):
            keys = OH.key_list(L, g)
            for w0 in range(a, b, 32):
                pos = np.arange(w0, min(w0 + 32, b))
                Q, K = c.wave_operands(h, L.written[pos], keys)
                s = Q @ K.T
                best = np.zeros(s.shape, dtype=bool)
                for i, p in enumerate(pos):
                    best[i, c.choice[p] if tied is None else list(tied[p])] = True
                top = s.max(1)
                chosen &= bool((np.where(best, s, top[:, None]) == top[:, None]).all())
                if not best.all():
                    worst = min(worst, float((top - np.where(best, -np.inf, s).max(1)).min()))
    return worst, chosen


# -------------------------------------------------------------------------------------------------------------- the ties
# 2 and 4 keys hold one k row and different v bytes (the integers 1 .. 16: the sums of four stay below 2^7 and their
# means are multiples of 1/4, exact in float32 and in both 16-bit types).  320 rows, 300 keys: 4 whole blocks and 44 keys;
# with 3 splits the boundaries are at keys 128 and 256.
#
# The mx and i8 kernels move a wave's reference point by WHOLE binades (the block exponent of the probabilities' scale), so
# a tied key that is not in the first block of its split is weighted 2^(z - m) with a fraction in the exponent, rounded to
# e4m3 -- within one split every tied key rounds alike and the mean is exact, across splits it is not (one part's weight
# carries the rounding, the other's does not).  TIES therefore gives every split that holds a tied key one in its first
# block, where m = z from the start; the all-e4m3 kernel moves the reference point to the block maximum itself and is also
# given TIES_FP8.
TIE_S, TIE_N_KV = 320, 300
TIES = ((33, 50),  # inside one 32-key group
        (31, 32),  # both sides of a 32-key edge
        (63, 64),  # both sides of a key-block edge
        (20, 127, 128, 140),  # both sides of a split boundary
        (10, 290),  # the first block and the partial last block
        (60, 190, 255, 256))  # four keys over three splits, both sides of the other boundary, the partial block included
TIES_FP8 = ((126, 129),  # both sides of a split boundary, neither in the first block of its split
            (100, 200, 250, 299))


def tie_sets(family):
    return TIES + (TIES_FP8 if family == "fp8" else ())


def tie_case(family, dtype, n_splits):
    """(Case, target): query row p attends the tied keys tie_sets(family)[target[p]]; expected: Case.expected(mean_of_best)"""
    L = plain_launch(1, TIE_S, TIE_S, TIE_N_KV, n_splits)
    sets = tie_sets(family)
    k = OH.keys_and_values(1, TIE_S)[0].copy()
    for t in sets:
        k[0, list(t)] = k[0, t[0]]
    rng = np.random.default_rng(5)
    target = rng.integers(0, len(sets), size=TIE_S)
    target[:len(sets)] = np.arange(len(sets))
    v8 = rng.choice(TIE_BYTES, size=(1, TIE_S, 128))
    seed = 1 + 2 * DTYPES.index(dtype)  # (odd: A = 5)
    c = Case(family, L, seed, dtype, v8=v8, k=k, choice=np.array([sets[t][0] for t in target]))
    return c, target


def mean_of_best(q_rows, k_rows, v_rows):
    """the `attend` of the ties: the mean of the v rows of the keys that share the best score"""
    s = q_rows @ k_rows.T
    best = s == s.max(1, keepdims=True)
    return (best @ v_rows) / best.sum(1, keepdims=True)
