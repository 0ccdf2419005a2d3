"""float64 restatement of vorta_sampled_fidelity (include/vorta_hip.h) and the comparison the GPU tests hold the kernel to.

Bounds (not fitted): the header states the longest chain of float32 roundings a sum passes through,
VORTA_SAMPLED_FIDELITY_CHAIN(n) = ceil(ceil(n / 16) / 16) + 19, and a row's own sum VORTA_SAMPLED_FIDELITY_ROW_CHAIN = 11;
every term is a square, so |sum - exact| <= CHAIN 2^-24 exact.  Maxima are exact: the float32 rounding of a difference is
monotone, so max |fl(d)| = fl(max |d|), the float64 maximum rounded once.  Non-finite results must be the float64
evaluation's (NaN where it has NaN, inf where it has inf), head by head; heads outside `heads` must hold `prefill`."""
import numpy as np

U = 2.0 ** -24
NAMES = ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err")


def f64(t):
    with np.errstate(invalid="ignore"):  # (rows no table names may hold anything, signalling NaNs of an unwritten buffer included)
        return t.detach().float().cpu().numpy().astype(np.float64)


def restate(ref, out, rows, heads=None):
    """ref (H, n, D), out (H, N, D) torch tensors, rows (n,) integers, heads: the measured heads (None: all).  float64
    statistics (H,) and row_sq_err (H, n); heads not measured are NaN"""
    x0, o = f64(ref), f64(out)
    H, n, D = x0.shape
    rows = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows, dtype=np.int64)
    heads = list(range(H)) if heads is None else [int(h) for h in heads]
    res = {name: np.full((H,), np.nan) for name in NAMES}
    res["row_sq_err"] = np.full((H, n), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in heads:
            a = x0[h].reshape(-1)
            d = (o[h][rows] - x0[h])
            res["sq_ref"][h] = (a * a).sum()
            res["sq_err"][h] = (d * d).sum()
            res["row_sq_err"][h] = (d * d).sum(1)
            if n:
                res["max_ref"][h], res["range_ref"][h], res["max_err"][h] = np.abs(a).max(), a.max() - a.min(), np.abs(d).max()
            else:
                res["max_ref"][h] = res["range_ref"][h] = res["max_err"][h] = 0.0
    return res, heads


def _close(got, want, bound, case, name):
    """relative bound where the exact value is positive, equality where it is zero or not finite; returns error / bound"""
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (case, name, got, want)
    zero = fin & (want == 0)
    assert (got[zero] == 0).all(), (case, name)
    pos = fin & (want > 0)
    ratio = np.abs(got[pos] - want[pos]) / (bound * want[pos])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (case, name, worst)
    return worst


def check(fid, ref, out, rows, heads=None, case="", prefill=None, chain_extra=0):
    """`fid` (ops.SampledFidelity) against the restatement on the same tensors.  Unmeasured heads: NaN, or `prefill` where the
    caller filled the buffers.  chain_extra: further roundings the caller's own combination adds.  Returns the largest
    error over bound of the sums."""
    from vorta_amd import _C
    want, heads = restate(ref, out, rows, heads)
    H, n, D = ref.shape
    bound = (_C.sampled_fidelity_chain(n) + chain_extra) * U
    assert bound < 1e-4, (n, bound)
    measured = np.zeros(H, dtype=bool)
    measured[heads] = True
    worst = 0.0
    for name in NAMES + (("row_sq_err",) if fid.row_sq_err is not None else ()):
        got = getattr(fid, name).double().cpu().numpy()
        w = want[name]
        if prefill is None:
            assert np.isnan(got[~measured]).all(), (case, name, "an unmeasured head is not NaN")
        else:
            assert (getattr(fid, name).cpu().numpy()[~measured] == np.float32(prefill)).all(), (case, name, "prefill changed")
        if name in ("sq_ref", "sq_err"):
            worst = max(worst, _close(got[measured], w[measured], bound, case, name))
        elif name == "row_sq_err":
            _close(got[measured], w[measured], _C.SAMPLED_FIDELITY_ROW_CHAIN * U, case, name)
        else:
            with np.errstate(over="ignore"):
                exact = w[measured].astype(np.float32)  # one rounding of the exact value
            assert np.array_equal(getattr(fid, name).cpu().numpy()[measured], exact, equal_nan=True), (case, name, got, w)
    assert fid.n == n * D
    print(f"{case}: n {n} chain {_C.sampled_fidelity_chain(n)} bound {bound:.3e} largest error / bound {worst:.4f}")
    return worst
