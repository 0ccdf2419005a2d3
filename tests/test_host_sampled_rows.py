"""CPU: `routed.sample_rows`, the stratified random table of video tokens on which the routed output is measured.

No phase lock (the bands are binomial, not fitted): at S = 118 800 (latent (33,45,80)) and n = 2 048 a token has odd `w` with
probability 1/2 -- 1 024 expected, sigma = sqrt(2048 / 4) = 22.6, band 1 024 +- 4 sigma = [933, 1115]; it is the centre of a
(2,3,2) coreset window (t odd and below 32, h = 1 mod 3, w odd) with probability (16/33)(1/3)(1/2) = 0.0808 -- 165.5 expected,
sigma 12.3, band [116, 215].  A table with a fixed stride would put every row, or none, on such a phase."""
import numpy as np
import pytest
import torch

from vorta_amd.routed import sample_rows

LATENT = (33, 45, 80)
S_HY = 33 * 45 * 80


@pytest.mark.parametrize("S,n", [(384, 48), (384, 1), (378, 64), (1000, 7), (S_HY, 2048), (8320, 1024)])
@pytest.mark.parametrize("seed", [0, 1, 1234])
def test_ascending_distinct_one_per_stratum_and_repeatable(S, n, seed):
    t = sample_rows(S, n, seed)
    assert t.dtype == torch.int32 and t.shape == (n,) and not t.is_cuda
    a = t.numpy().astype(np.int64)
    i = np.arange(n, dtype=np.int64)
    lo, hi = (i * S) // n, ((i + 1) * S) // n
    assert (a >= lo).all() and (a < hi).all()            # one per stratum ...
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < S  # ... hence ascending, distinct, inside [0, S)
    u = np.random.default_rng(seed).random(n)
    assert np.array_equal(a, lo + np.floor(u * (hi - lo)).astype(np.int64))  # the documented draw
    assert sample_rows(S, n, seed) is t                   # built once
    if n > 1 and S > 2 * n:
        assert not np.array_equal(a, sample_rows(S, n, seed + 1).numpy())


def test_all_rows_none_and_too_many():
    assert sample_rows(384, 384).tolist() == list(range(384))
    assert sample_rows(384, 384, seed=5).tolist() == list(range(384))
    assert sample_rows(384, 0).shape == (0,)
    with pytest.raises(ValueError):
        sample_rows(384, 385)


@pytest.mark.parametrize("seed,odd_w,centres", [(0, 1024, 169), (1, 1011, 159), (1234, 1054, 181)])
def test_no_phase_lock_at_hunyuan_129f(seed, odd_w, centres):
    a = sample_rows(S_HY, 2048, seed).numpy().astype(np.int64)
    w, h, t = a % 80, (a // 80) % 45, a // (80 * 45)
    n_odd = int((w % 2 == 1).sum())
    n_centre = int(((t % 2 == 1) & (t < 32) & (h % 3 == 1) & (w % 2 == 1)).sum())
    print(f"seed {seed}: {n_odd} rows on odd w, {n_centre} coreset-window centres")
    assert 933 <= n_odd <= 1115 and 116 <= n_centre <= 215
    assert (n_odd, n_centre) == (odd_w, centres)  # this numpy draw, recorded
    # every frame is seen: 33 frames of 3 600 tokens, strata of 58 tokens
    assert set(t.tolist()) == set(range(33))
