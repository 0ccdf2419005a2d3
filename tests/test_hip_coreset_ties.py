"""vorta_coreset_select where its ranking has to break ties and at the limits of its window: keep / drop / key-side lists against
a numpy stable ascending argsort of float64 similarities, index for index, with no mask of "clear" groups.  The inputs make every
tie exact -- duplicated rows have the same bits, so they get the same similarity in any arithmetic -- and every other pair of
similarities of a group lies further apart than fp32 can blur (asserted on the float64 reference, for the fixed seeds).

Heads of one launch: 0 every token the same row; 1 all zeros (the 1e-12 clamp: no NaN, order = margin order); 2 each group's margins
in bit-identical pairs (margin m and m + ceil(nm / 2)); 3 distinct rows."""
import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O
from _util import dev

pytestmark = pytest.mark.gpu

#          window      latent      (groups)
WINDOWS = {(4, 4, 4): (4, 8, 4),   # 64 tokens = MAX_G, 63 margins: bit 63 of the key-side ballot, four prefetch rounds
           (3, 3, 3): (3, 6, 3),
           (1, 1, 2): (2, 3, 4),   # one margin
           (2, 1, 1): (4, 3, 2)}   # one margin, the centre is the window's LAST token
N_TAIL = 3
PAD = 5  # physical rows more than tokens, so that a row_map is not a permutation of the token ids
MIN_GAP = 1e-5  # fp32 similarities of 128 channels are good to ~1e-6


SEEDS = {(4, 4, 4): 1, (3, 3, 3): 0, (1, 1, 2): 0, (2, 1, 1): 0}  # draws without near-ties in either dtype (_reference asserts it)


def _inputs(window, dtype, seed=None):
    latent = WINDOWS[window]
    gi = O.group_info(latent, window)
    S, G, nm = latent[0] * latent[1] * latent[2], gi.n_groups, gi.margin.shape[1]
    g = torch.Generator().manual_seed(SEEDS[window] if seed is None else seed)
    x = torch.randn((4, S + N_TAIL, 128), generator=g)
    x[0] = x[0, 0]
    x[1] = 0
    half = -(-nm // 2)
    for grp in range(G):
        for m in range(half, nm):
            x[2, gi.margin[grp, m]] = x[2, gi.margin[grp, m - half]]
    return latent, gi, x.to(dtype)


def _reference(gi, x):
    """per head: (stable ascending order of the margins (G,nm), float64 similarities)"""
    sims = O.coreset_similarity(x.double().numpy()[None], gi)[0]  # (4,G,nm)
    assert np.isfinite(sims).all()
    d = np.diff(np.sort(sims, axis=-1), axis=-1)
    assert ((d == 0) | (d > MIN_GAP)).all(), "the fixed inputs must not hold near-ties"
    assert (d[0] == 0).all() and (d[1] == 0).all() and (sims[1] == 0).all()
    if sims.shape[-1] > 1:
        assert ((d[2] == 0).sum(-1) == sims.shape[-1] // 2).all() and (d[3] > 0).all()
    return np.argsort(sims, axis=-1, kind="stable")


def _expected(gi, order, head, n_keep, row_of, S):
    """(keep (G(1+nk)+tail,), drop (G, nm-nk), key-side (G(1+nk)+tail,)) of one head"""
    G = gi.n_groups
    kept = np.take_along_axis(gi.margin, order[head][:, :n_keep], axis=1)   # token ids, least similar first
    dropped = np.take_along_axis(gi.margin, order[head][:, n_keep:], axis=1)
    tail = np.arange(S, S + N_TAIL)
    keep = np.concatenate([gi.center[:, 0], kept.reshape(-1), tail])
    kv = np.concatenate([np.sort(np.concatenate([gi.center, kept], axis=1), axis=1).reshape(-1), tail])
    return row_of[keep], row_of[dropped], row_of[kv]


@pytest.mark.parametrize("which_keep", ["0", "1", "g-2", "g-1"])
@pytest.mark.parametrize("window", list(WINDOWS), ids=lambda w: "x".join(map(str, w)))
def test_coreset_exact_ties(window, which_keep):
    from vorta_amd import ops
    g = window[0] * window[1] * window[2]
    n_keep = {"0": 0, "1": 1, "g-2": g - 2, "g-1": g - 1}[which_keep]
    dtype = torch.bfloat16 if (g + n_keep) % 2 else torch.float16
    latent, gi, x = _inputs(window, dtype)
    S, G, nm = latent[0] * latent[1] * latent[2], gi.n_groups, g - 1
    order = _reference(gi, x)
    perm = torch.randperm(S + N_TAIL + PAD, generator=torch.Generator().manual_seed(g))[: S + N_TAIL]
    x_phys = torch.zeros((4, S + N_TAIL + PAD, 128), dtype=dtype)
    x_phys[:, perm] = x
    for use_map in (False, True):
        xd = (x_phys if use_map else x).to(dev())
        row_map = perm.int().to(dev()) if use_map else None
        row_of = perm.numpy() if use_map else np.arange(S + N_TAIL)
        for heads in (None, [2, 0, 3, 1]):
            hl = None if heads is None else torch.tensor(heads, dtype=torch.int32, device=dev())
            for want_kv in (False, True):
                res = ops.coreset_select(xd, latent, window, n_keep, head_list=hl, tail_first=S, n_tail=N_TAIL, row_map=row_map,
                                         want_kv=want_kv)
                torch.cuda.synchronize()
                keep, drop = res[0].cpu().numpy(), res[1].cpu().numpy()
                assert keep.shape == (4, G * (1 + n_keep) + N_TAIL) and drop.shape == (4, G, nm - n_keep)
                for y, h in enumerate(heads or range(4)):
                    what = (window, n_keep, use_map, heads, want_kv, y, h)
                    keep_ref, drop_ref, kv_ref = _expected(gi, order, h, n_keep, row_of, S)
                    assert np.array_equal(keep[y], keep_ref), what
                    assert np.array_equal(drop[y], drop_ref), what
                    # centre + kept + dropped = the window, once each
                    rows = np.concatenate([keep[y, :G, None], keep[y, G:G + G * n_keep].reshape(G, n_keep), drop[y]], axis=1)
                    groups = np.concatenate([gi.center, gi.margin], axis=1)
                    assert np.array_equal(np.sort(rows, axis=1), np.sort(row_of[groups], axis=1)), what
                    if want_kv:
                        assert np.array_equal(res[2].cpu().numpy()[y], kv_ref), what


def test_coreset_refuses_a_65_token_window():
    from vorta_amd import _C, ops
    x = torch.zeros((1, 65, 128), dtype=torch.bfloat16, device=dev())
    with pytest.raises(_C.VortaHipError):
        ops.coreset_select(x, (5, 13, 1), (5, 13, 1), 3)
