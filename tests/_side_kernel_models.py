"""The yardsticks of the router and norm+RoPE shape tests: float64 ROUNDING MODELS of vorta_router_route and vorta_qk_norm_rope
(include/vorta_hip.h:549-606) with a derived bound per output element, written from the header and the formulae
(tests/test_host_side_kernel_models.py, tests/test_hip_router_shapes.py, tests/test_hip_norm_rope_shapes.py).

Each model is the float64 operation with exactly the roundings to the 16-bit I/O type T that the kernels make by design:

    router      s = round_T(silu(temb))                      csrc/router.hip:46,51
                logit = round_T(s . W + b)                   csrc/router.hip:56   (the model keeps logit64 and bounds the rounding)
                score = round_T(softmax(logit))              csrc/router.hip:77
    norm+RoPE   out = round_T(rope(rms_norm(x) w))           csrc/qk_norm_rope.hip:88-93,153-158   (one rounding, at the store)
                eps is a float of the argument block         include/vorta_hip.h:602

Everything between those roundings is fp32 in the kernels and float64 here; the bounds charge that difference.  With the
roundings off the models are oracle.vorta_oracle.router_scores and O.rope_interleaved(O.rms_norm(.)).  The fp32 numpy
RESTATEMENTS below (and their deliberately truncated variants) exist to show on a CPU that the bounds are attainable and
that a kernel which reads less than it should lands outside them.  Nothing here loads the library."""
import os

import numpy as np
import torch

from oracle import vorta_oracle as O

U32 = 2.0 ** -24  # unit roundoff of fp32
# __expf has no stated error in this project: a silu value whose float64 value, moved by 16 fp32 ulps either way, rounds to a
# different T is allowed to round either way in the kernel.  One named constant; a logit outside its bound that a wider
# allowance would admit is a finding, not a reason to raise it.
EXPF_ALLOWANCE = 2.0 ** -20

#            significand bits, frexp exponent of the smallest normal, largest finite
_FORMAT = {torch.bfloat16: (8, -125, float.fromhex("0x1.fep127")),
           torch.float16: (11, -13, 65504.0),
           torch.float32: (24, -125, float.fromhex("0x1.fffffep127"))}


def dtype_name(dtype):
    return str(dtype).split(".")[-1]


def ulp_T(x, dtype):
    """spacing of T at |x| (of the subnormals below the smallest normal), float64"""
    p, emin, _ = _FORMAT[dtype]
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(x)[1]
    e = np.where(x == 0, emin, np.maximum(e, emin))
    return np.ldexp(1.0, e - p)


def round_T(x, dtype):
    """float64 -> nearest T (ties to even, one rounding, subnormals kept, overflow to inf) -> float64"""
    x = np.asarray(x, dtype=np.float64)
    q = ulp_T(x, dtype)
    r = np.rint(x / q) * q
    return np.where(np.abs(r) > _FORMAT[dtype][2], np.copysign(np.inf, x), r)


def _silu64(x):
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


# ------------------------------------------------------------------------------------------------ router
class RouterModel:
    """logit64 (B,H,3), scores64 (B,H,3), delta (B,H,3): see router_model"""

    def __init__(self, dtype, s, logit64, delta):
        self.dtype, self.s, self.logit64, self.delta = dtype, s, logit64, delta
        y = logit64 - logit64.max(-1, keepdims=True)
        e = np.exp(y)
        self.scores64 = e / e.sum(-1, keepdims=True)
        # bounds that need no kernel output (the clarity condition is decided on the reference alone): a logit inside its
        # bound lies at most ulp_T(logit64) + delta beyond |logit64|, so this is no smaller than logit_bound(got)
        self.lb_ref = 0.5 * ulp_T(np.abs(logit64) + ulp_T(logit64, dtype) + delta, dtype) + delta
        self.sb_ref = self.score_bound(None)

    def logit_bound(self, got=None):
        """lb = 0.5 ulp_T(max(|logit64|, |got|)) + delta: the one rounding of csrc/router.hip:56 plus the fp32 sum"""
        if got is None:
            return self.lb_ref
        return 0.5 * ulp_T(np.maximum(np.abs(self.logit64), np.abs(np.asarray(got, np.float64))), self.dtype) + self.delta

    def score_bound(self, got_logits=None):
        """sb = scores64 (exp(2 max_e lb) - 1) + 0.5 ulp_T(scores64) (1 + 2^-6): logits moved by at most L = max_e lb move a
        softmax value by a factor within exp(+-2L); the second term is the rounding of csrc/router.hip:77 with 2^-6 of it for
        the fp32 exp, sum and division in front"""
        L = self.logit_bound(got_logits).max(-1, keepdims=True)
        return self.scores64 * np.expm1(2.0 * L) + 0.5 * ulp_T(self.scores64, self.dtype) * (1.0 + 2.0 ** -6)

    def route64(self, tau):
        """the float64 route of batch item 0 with tau rounded to T (csrc/router.hip:82-84)"""
        return O.route_heads(self.scores64, float(round_T(tau, self.dtype)))

    def clear_heads(self, tau):
        """heads whose route cannot depend on rounding: batch item 0's top score beats the runner-up by more than
        2 max_e sb and lies more than that from round_T(tau)"""
        s = np.sort(self.scores64[0], axis=-1)
        m = 2.0 * self.sb_ref[0].max(-1)
        return (s[:, -1] - s[:, -2] > m) & (np.abs(s[:, -1] - float(round_T(tau, self.dtype))) > m)


def router_model(temb, W, b, heads, dtype, roundings=True):
    """temb (B,E), W (heads*3,E), b (heads*3,): values of T (float arrays or tensors).

        s = round_T(silu64(temb))                                            csrc/router.hip:46
        logit64 = s . W + b   in float64
        delta = (E/64 + 8) 2^-24 (sum |s_i w_i| + |b|) + sum_flip ulp_T(s_i) |w_i|

    The first term of delta is the fp32 summation: E/64 sequential adds per lane (csrc/router.hip:40-47), the 6-step butterfly
    (:54) and the bias add (:56), each at most 2^-24 of the running magnitude, with the products' own roundings and slack in the
    8.  The second covers silu values so close to a rounding midpoint of T that the fp32 silu may round the other way: element i
    is `flip` when round_T(silu64 (1 +- EXPF_ALLOWANCE)) differ, and then costs one ulp_T(s_i) times |w_i|."""
    as64 = lambda a: (a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64))
    temb, W, b = as64(temb), as64(W), as64(b)
    B, E = temb.shape
    sil = _silu64(temb)
    if roundings:
        s = round_T(sil, dtype)
        flip = round_T(sil * (1 + EXPF_ALLOWANCE), dtype) != round_T(sil * (1 - EXPF_ALLOWANCE), dtype)
        flip_w = flip * ulp_T(s, dtype)
    else:
        s, flip_w = sil, np.zeros_like(sil)
    logit64 = s @ W.T + b
    absum = np.abs(s) @ np.abs(W).T + np.abs(b)
    delta = (E / 64 + 8) * U32 * absum + flip_w @ np.abs(W).T
    shape = (B, heads, -1)
    return RouterModel(dtype, s, logit64.reshape(shape), delta.reshape(shape))


def to_T32(x, dtype):
    """fp32 numpy -> T -> fp32 numpy, by torch's own conversion"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def router_restate_f32(temb, W, b, heads, dtype, drop_last=0):
    """fp32 numpy restatement of the router arithmetic: silu in fp32 rounded to T, fp32 matmul, logit rounded to T, fp32
    softmax rounded to T.  Returns (logits (B,H,3), scores (B,H,3)) as fp32 arrays of T values.  `drop_last` leaves that many
    trailing elements out of the dot product: what a kernel whose loop stops early computes."""
    x = np.asarray(temb, np.float32)
    with np.errstate(over="ignore"):
        s = to_T32(x / (np.float32(1) + np.exp(-x)), dtype)
    E = x.shape[1] - drop_last
    acc = s[:, :E] @ np.asarray(W, np.float32)[:, :E].T if E > 0 else np.zeros((x.shape[0], len(b)), np.float32)
    lg = to_T32(acc + np.asarray(b, np.float32), dtype).reshape(x.shape[0], heads, -1)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return lg, to_T32(e / e.sum(-1, keepdims=True, dtype=np.float32), dtype)


# (dtype, batch, E, H), the seed and the bias spread of tests/test_hip_router_shapes.py; seeds and spreads are chosen so that
# the clarity condition holds (test_host_side_kernel_models.py::test_unclear_heads_within_the_cap proves it)
ROUTER_CASES = {
    "a": (torch.bfloat16, 2, 3072, 24),   # Hunyuan
    "b": (torch.float16, 2, 5120, 40),    # Wan-14B with guidance: 80 items, a second trip of the route loop
    "c": (torch.bfloat16, 1, 8, 3),       # one lane does all the work; the last workgroup holds one live wave
    "d": (torch.float16, 1, 520, 6),      # a second trip of the vector loop taken by lane 0 alone
    "e": (torch.bfloat16, 1, 1024, 1024),  # the limit of s_expert
    "f": (torch.float16, 3, 512, 70),
}
ROUTER_DRAW = {"a": (0, 2.0), "b": (0, 2.0), "c": (0, 4.0), "d": (0, 2.0), "e": (0, 2.0), "f": (0, 2.0)}  # seed, bias spread
ROUTER_TAUS = (0.0, 0.5, 0.9)
PLANTED_CASE = "d"
PLANTED = (120.0, -120.0, 20.0, -20.0, 0.0)


def router_inputs(case, layers=None, draw=None):
    """(temb (B,E), W ([L,]3H,E), b ([L,]3H)) tensors of the case's dtype on the CPU: temb ~ 1.5 N(0,1), W ~ N(0,1) / sqrt(E),
    b ~ spread N(0,1)"""
    dtype, B, E, H = ROUTER_CASES[case]
    seed, spread = draw or ROUTER_DRAW[case]
    g = torch.Generator().manual_seed(1000 * (ord(case) - ord("a")) + seed)
    lead = () if layers is None else (layers,)
    temb = 1.5 * torch.randn((B, E), generator=g)
    W = torch.randn(lead + (3 * H, E), generator=g) / E ** 0.5
    b = spread * torch.randn(lead + (3 * H,), generator=g)
    if case == PLANTED_CASE:
        temb[0, 1:1 + len(PLANTED)] = torch.tensor(PLANTED)
    return temb.to(dtype), W.to(dtype), b.to(dtype)


def unclear_cap(H):
    return max(1, H // 4)


# ------------------------------------------------------------------------------------------------ norm + RoPE
def norm_rope_slack(heads, across_heads):
    """slack = (k/2 + 8) 2^-24 with k the fp32 additions on the longest path of the sum of squares: 8 in-lane adds and the
    4-step quarter-wave butterfly for the per-head kernel (csrc/qk_norm_rope.hip:79-80), 8 per 16-byte chunk of the lane,
    ceil(heads 16 / 64) chunks, and the 6-step butterfly across heads (:123-133)"""
    k = 8 * -(-heads * 16 // 64) + 6 if across_heads else 12
    return (k / 2 + 8) * U32


def norm_rope_model(x, w, eps, cos, sin, rope_tokens, across_heads):
    """float64 O.rms_norm then O.rope_interleaved of x (H,S,D) = the call's rows as float64 values of T; w (D,), (H*D,) or
    None; cos / sin (>= rope_tokens, D) or None.  Returns (ref, mag), both (H,S,D):

        bound = 0.5 ulp_T(max(|ref|, |got|)) + slack mag,    mag = |y_a c| + |y_b s| on rotated rows, |y| on the others

    Derivation: the sum of squares is a sum of non-negative fp32 terms, so k additions and one product rounding leave a relative
    error of at most (k + 1) 2^-24, of which rsqrt passes on half; the scaling by 1/D, the eps add and rsqrtf itself (2 ulp)
    add at most 3 2^-24 more to r; y = x r w is two roundings, each product with cos / sin one, their sum or difference one,
    relative to |y_a c| + |y_b s| because the two products may cancel: (k + 1)/2 + 3 + 4 <= k/2 + 8.  Then the one rounding to
    T at the store.  A row dominated by eps only makes the first part smaller."""
    x = np.asarray(x, np.float64)
    H, S, D = x.shape
    eps = float(np.float32(eps))
    if across_heads:
        y = O.rms_norm(x.transpose(1, 0, 2).reshape(S, H * D), w, eps).reshape(S, H, D).transpose(1, 0, 2)
    else:
        y = O.rms_norm(x, w, eps)
    ref, mag = y.copy(), np.abs(y)
    R = rope_tokens if cos is not None else 0
    if R:
        c, s = np.asarray(cos, np.float64)[:R], np.asarray(sin, np.float64)[:R]
        ref[:, :R] = O.rope_interleaved(y[:, :R], c, s)
        partner = y[:, :R].reshape(H, R, D // 2, 2)[..., ::-1].reshape(H, R, D)
        mag[:, :R] = np.abs(y[:, :R] * c) + np.abs(partner * s)
    return ref, mag


def norm_rope_bound(ref, mag, got, heads, across_heads, dtype):
    return 0.5 * ulp_T(np.maximum(np.abs(ref), np.abs(np.asarray(got, np.float64))), dtype) + norm_rope_slack(heads, across_heads) * mag


def norm_rope_restate_f32(x, w, eps, cos, sin, rope_tokens, across_heads, dtype, skip=None):
    """fp32 numpy restatement of the kernel: fp32 sum of squares, r = 1 / sqrt(mean + eps), y = x r w, rotation, one rounding
    to T.  skip="chunk" leaves the last 16-byte chunk (8 channels) of every row out of the sum of squares, skip="head" the last
    head of the across-heads sum: kernels that read less than they should."""
    x = np.asarray(x, np.float32)
    H, S, D = x.shape
    sq = x * x
    if skip == "chunk":
        sq = sq[..., :D - 8]
    if across_heads:
        if skip == "head":
            sq = sq[:H - 1]
        ss = sq.sum(axis=(0, 2), dtype=np.float32)[None, :, None]
        n = H * D
    else:
        ss = sq.sum(axis=-1, dtype=np.float32)[..., None]
        n = D
    r = np.float32(1) / np.sqrt(ss / np.float32(n) + np.float32(eps), dtype=np.float32)
    y = x * r
    if w is not None:
        y = y * np.asarray(w, np.float32).reshape((H, 1, D) if across_heads else (1, 1, D))
    out = y.copy()
    R = rope_tokens if cos is not None else 0
    if R:
        c, s = np.asarray(cos, np.float32)[:R], np.asarray(sin, np.float32)[:R]
        ya, yb = y[:, :R, 0::2], y[:, :R, 1::2]
        out[:, :R, 0::2] = ya * c[:, 0::2] - yb * s[:, 0::2]
        out[:, :R, 1::2] = yb * c[:, 1::2] + ya * s[:, 1::2]
    return to_T32(out, dtype)


# A covering subset of {dtype} x {weight, None} x {rope_tokens 0, odd in the middle, all} x {token_offset 0, 3} x
# {n_tokens 1, 5, 7, 64} per kernel: (dtype, heads, n_tokens, token_offset, rope_tokens, weight, layout); layout "hsd" is the
# contiguous (H,S,D) tensor, "shd" the (S,H*D) projection output viewed as (H,S,D).
#   per head (csrc/qk_norm_rope.hip:69): 24 heads per trip -- 25 puts one quarter wave into a second trip, 49 into a third;
#   n_tokens % 4 != 0 leaves a partly filled workgroup (:51)
#   across heads (:101-175): 1 leaves 48 lanes idle, 5 and 13 make `c < chunks` partly true, 13 and 25 select the next MAXIT
_BF, _FP = torch.bfloat16, torch.float16
NORM_ROPE_CASES = {
    False: [(_BF, 1, 1, 0, 1, True, "hsd"), (_FP, 3, 5, 3, 3, False, "shd"), (_BF, 4, 7, 0, 0, True, "shd"),
            (_FP, 24, 64, 3, 33, True, "hsd"), (_BF, 25, 5, 3, 5, False, "shd"), (_FP, 29, 7, 0, 3, True, "shd"),
            (_BF, 49, 64, 3, 64, True, "shd")],
    True: [(_FP, 1, 5, 3, 5, True, "shd"), (_BF, 5, 7, 0, 3, False, "shd"), (_FP, 12, 1, 0, 0, True, "hsd"),
           (_BF, 13, 64, 3, 33, True, "shd"), (_FP, 24, 7, 3, 7, False, "shd"), (_BF, 25, 5, 0, 3, True, "hsd"),
           (_FP, 40, 64, 0, 64, True, "shd")],
}
NORM_ROPE_EPS = 1e-6


def norm_rope_case_id(across_heads, case):
    dtype, H, n, off, rope, weight, layout = case
    return f"{'across' if across_heads else 'per_head'}-{dtype_name(dtype)}-H{H}-n{n}-off{off}-rope{rope}-{'w' if weight else 'now'}-{layout}"


def norm_rope_inputs(across_heads, case, seed=0):
    """(x (H,n,D) the call's rows, w or None, cos, sin (n,D) fp32) on the CPU: x ~ 2 N(0,1) in T, w ~ U(0.5, 1.5) in T"""
    dtype, H, n, off, rope, weight, layout = case
    g = torch.Generator().manual_seed(seed + 7 * H + n)
    x = (2 * torch.randn((H, n, 128), generator=g)).to(dtype)
    w = (torch.rand(H * 128 if across_heads else 128, generator=g) + 0.5).to(dtype) if weight else None
    ang = torch.rand((n, 64), generator=g) * 6.28
    return x, w, ang.cos().repeat_interleave(2, dim=1).contiguous(), ang.sin().repeat_interleave(2, dim=1).contiguous()


def special_rows(across_heads, dtype, H=5, n=8):
    """x (H,n,D) ~ 2 N(0,1) in T with, per head row (or, across heads, per whole token) 0..3: all zeros; values that eps
    dominates (fp16 subnormals / bf16 1e-20); one-hot; for fp16, +-3e4 in every channel (sum of squares ~1e11 per head)"""
    g = torch.Generator().manual_seed(11)
    x = (2 * torch.randn((H, n, 128), generator=g)).to(dtype)
    sign = torch.where(torch.rand((H, 128), generator=g) < 0.5, -1.0, 1.0)
    tiny = (6e-8 * torch.randint(1, 900, (H, 128), generator=g) if dtype == torch.float16 else 1e-20 * (1 + torch.rand((H, 128), generator=g)))
    rows = [torch.zeros(H, 128), tiny * sign, torch.zeros(H, 128), 3e4 * sign]
    rows[2][H - 1 if across_heads else slice(None), 77] = -1.5
    for t, r in enumerate(rows[:4 if dtype == torch.float16 else 3]):
        if across_heads:
            x[:, t] = r.to(dtype)
        else:
            x[t % H, t] = r[0].to(dtype)
    return x


# ------------------------------------------------------------------------------------------------ the record
def write_record_section(title, lines):
    """print the section; when VORTA_SIDE_KERNELS_ACCURACY_OUT names a file (profiles/side_kernels_accuracy.txt comes from
    there), put it into that file in place of an earlier section of the same title"""
    print("\n".join([title] + lines))
    path = os.environ.get("VORTA_SIDE_KERNELS_ACCURACY_OUT")
    if not path:
        return
    head = ("worst error / bound of the router and norm+RoPE kernels against the rounding models of "
            "tests/_side_kernel_models.py (every value must be at most 1)")
    sections = {}
    if os.path.exists(path):
        cur = None
        for ln in open(path).read().splitlines()[1:]:
            if ln.startswith("== "):
                cur = ln
                sections[cur] = []
            elif cur is not None:
                sections[cur].append(ln)
    sections["== " + title] = lines
    with open(path, "w") as f:
        f.write(head + "\n")
        for t in sorted(sections):
            f.write("\n".join([t] + sections[t]) + "\n")
