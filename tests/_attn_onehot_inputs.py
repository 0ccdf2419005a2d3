"""Inputs on which the attention forward is exact (tests/test_hip_attention_onehot.py, tests/test_host_forward_model.py):
every query's softmax is ONE key, so its output row is that key's v row with every bit equal, whatever the routing tables
(q_rows, kv_rows, groups, q_block_table, dup_rows, splits) do.

    k = 5 x (+-1 sign vectors), drawn once per (H, S);  v = integers in [-64, 64];  q[h, row of position p] = k[h, key chosen
    for p], the key taken among the first n_kv_eff entries of the key list of p's own group;  scale = 128^-0.5.

The matching key scores 128 x 5 x round16(5 scale log2 e), about 408 log2 units; any other sign vector agrees with it on
fewer than 100 of 128 coordinates more than the mean, and `best_key_gaps` measures what is left: the tests assert >= 160 log2
units before any launch.  Every other probability and every rescale factor is then exp2(<= -160) = 0 in float32, the row sum
is 1 and the products are the integers of v.  Nothing here reads the library."""
import functools

import numpy as np
import torch

KVB = 64
LOG2E = 1.4426950408889634
SCALE = 128 ** -0.5
MIN_GAP = 160.0


@functools.lru_cache(maxsize=None)
def keys_and_values(H, S):
    """(k, v) as (H,S,128) float64 numpy arrays, exact in bf16 and fp16"""
    rng = np.random.default_rng(1000 * H + S)
    return 5.0 * rng.choice([-1.0, 1.0], size=(H, S, 128)), rng.integers(-64, 65, size=(H, S, 128)).astype(np.float64)


def key_list(L, g):
    """row ids of the effective keys of group g of launch L (tests/_random_launch.py)"""
    keys = L.kv_rows[g if L.per_group else 0] if L.kv_rows is not None else np.arange(L.kv_off, L.kv_off + L.n_kv)
    return np.asarray(keys[:L.n_kv_eff])


def forced_choices(L):
    """key positions every group's queries must choose among their first ones: 0, the last effective key, 63 / 64, the last
    position of every split and the first of the next (split boundaries are cut from the host n_kv)"""
    bps = -(-(-(-L.n_kv // KVB)) // L.n_splits)
    want = [0, L.n_kv_eff - 1, 63, 64]
    for s in range(1, L.n_splits):
        want += [s * bps * KVB - 1, s * bps * KVB]
    return sorted({c for c in want if 0 <= c < L.n_kv_eff})


def inputs(L, seed=0):
    """(q, k, v, choice) of launch L: float64 numpy (H_buf,S,128) arrays, and choice[h][p] = index into the key list of p's
    group of the key position p attends (the same for every head: the heads differ in k and v)"""
    rng = np.random.default_rng(50_000 + seed)
    k, v = keys_and_values(L.H_buf, L.S)
    q = 5.0 * rng.choice([-1.0, 1.0], size=k.shape)  # rows no launch names still hold sign vectors
    choice = rng.integers(0, L.n_kv_eff, size=L.n_q)
    forced = forced_choices(L)
    for a, b in L.bounds:
        n = min(len(forced), b - a)
        choice[a:a + n] = forced[:n]
        if b - a >= 2:  # a short group still reaches the last key and position 0
            choice[b - 1] = L.n_kv_eff - 1
    for g, (a, b) in enumerate(L.bounds):
        keys = key_list(L, g)
        for h in range(L.H_buf):
            q[h, L.written[a:b]] = k[h, keys[choice[a:b]]]
    return q, k, v, choice


def best_key_gaps(L, q, k, choice, scale_log2):
    """(smallest lead of the best key over the second, in log2 units, over every row the launch computes; whether the best
    key is the chosen one on every such row) from float64 scores"""
    worst, chosen = np.inf, True
    for h in L.live:
        for g, (a, b) in enumerate(L.bounds):
            keys = key_list(L, g)
            s = (q[h, L.written[a:b]] @ k[h, keys].T) * scale_log2
            chosen &= bool((s.argmax(1) == choice[a:b]).all())
            if len(keys) > 1:
                top = np.sort(s, axis=1)
                worst = min(worst, float((top[:, -1] - top[:, -2]).min()))
    return worst, chosen


def pick_chosen(q_rows, k_rows, v_rows):
    """the `attend` of RL.dense_reference: every query's output is the v row of its best key"""
    return v_rows[(q_rows @ k_rows.T).argmax(1)].copy()


def tensors(dtype, device, *arrays):
    return tuple(torch.as_tensor(a, dtype=torch.float64).to(dtype).to(device) for a in arrays)
