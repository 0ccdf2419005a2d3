"""GPU, bit for bit: the 16-bit attention forward (csrc/attn_fwd.hip) on inputs whose every softmax row is ONE key
(tests/_attn_onehot_inputs.py).  The output row of a query is then the v row of its key with every bit equal, so the routing
of a launch -- q_rows, kv_rows, groups, q_block_table, dup_rows, head lists, device lengths, key splits and their merge -- is
checked exactly, not within a tolerance: a key list read one entry off, a row of one lane written to another, a split merged
with the wrong weight all change bits.

Random launches: tests/_random_launch.py's, both dtypes and both kernels (variant 0: pipelined; 1: plain), `torch.equal`
against RL.dense_reference on the whole buffer, the sentinel rows included.  The chosen keys include position 0, the last
effective key, 63 / 64 and both sides of every split boundary.

Ties: 2 and 4 keys hold one k row and different integer v rows; the output is round16((v_a + v_b) / 2), respectively / 4 --
exact, because l is 2 or 4 and the sums are integers below 2^8."""
import numpy as np
import pytest
import torch

import _attn_onehot_inputs as OH
import _random_launch as RL
from _util import dev

pytestmark = pytest.mark.gpu

N_SEEDS = 32
DTYPES = (torch.bfloat16, torch.float16)


def _draw(seed):
    return RL.draw(np.random.default_rng(9300 + seed), S_range=(64, 600))


def _scale_log2(dtype):
    """what one coordinate of q k contributes: 5 x round16(5 scale log2 e), per unit of +-1 agreement"""
    return float(torch.tensor(5.0 * OH.SCALE * OH.LOG2E).to(dtype)) / 5.0


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_launches_write_the_chosen_v_rows(seed):
    from vorta_amd import ops
    L = _draw(seed)
    dtype, variant = DTYPES[seed % 2], (seed // 2) % 2
    q, k, v, choice = OH.inputs(L, seed)
    gap, chosen = OH.best_key_gaps(L, q, k, choice, _scale_log2(dtype))  # a check of the inputs, before any launch
    print(f"seed {seed} {RL.describe(L)} variant {variant}: smallest lead of the best key {gap:.1f} log2 units")
    assert chosen and gap >= OH.MIN_GAP
    want = torch.as_tensor(RL.dense_reference(L, q, k, v, OH.pick_chosen)).to(dtype)
    qd, kd, vd = OH.tensors(dtype, dev(), q, k, v)
    out = torch.full(qd.shape, RL.SENTINEL, dtype=dtype, device=dev())
    ops.attn_fwd(qd, kd, vd, out, scale=OH.SCALE, variant=variant, **RL.kwargs(L, dev()))
    torch.cuda.synchronize()
    got = out.cpu()
    bad = (got != want).any(-1).nonzero().tolist()
    assert torch.equal(got, want), f"seed {seed} {RL.describe(L)} variant {variant}: {len(bad)} rows differ, first (head, row) {bad[:4]}"


def test_the_random_launches_reach_every_feature():
    """(needs no GPU work: what the 32 seeds above cover, among the launches that compute anything)"""
    seen = {}
    for seed in range(N_SEEDS):
        L = _draw(seed)
        if len(L.live) == 0 or L.q_valid_eff == 0:
            continue
        for name, on in (("splits", L.n_splits > 1), ("q_rows", L.q_rows is not None), ("kv_rows", L.kv_rows is not None),
                         ("q_block_table", L.qtab is not None), ("duplicates", L.n_dup_pos > 0),
                         ("device lengths", L.n_kv_dev is not None or L.q_valid_dev is not None),
                         ("split boundary chosen", L.n_splits > 1 and len(OH.forced_choices(L)) > 4)):
            seen[name] = seen.get(name, 0) + int(on)
    print(seen)
    assert all(seen.get(n, 0) >= 2 for n in ("splits", "q_rows", "kv_rows", "q_block_table", "duplicates", "device lengths",
                                             "split boundary chosen")), seen


# -------------------------------------------------------------------------------------------------------------- the ties
TIE_S, TIE_N_KV = 320, 300  # 4 whole blocks and 44 keys; with 3 splits the boundaries are at keys 128 and 256
TIES = ((70, 100),  # inside one block
        (10, 290),  # the first block and the partial last block
        (127, 128),  # both sides of a split boundary
        (60, 255, 256, 280),  # four keys over three splits, both sides of the other boundary, the partial block included
        (192, 200, 210, 254))  # four keys inside one block


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("n_splits", (1, 3))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_tied_keys_average_their_v_rows(dtype, n_splits, variant):
    from vorta_amd import ops
    k, v = (x.copy() for x in OH.keys_and_values(1, TIE_S))
    for t in TIES:
        k[0, list(t)] = k[0, t[0]]
    rng = np.random.default_rng(5)
    q = 5.0 * rng.choice([-1.0, 1.0], size=k.shape)
    target = rng.integers(0, len(TIES), size=TIE_S)
    target[:len(TIES)] = np.arange(len(TIES))
    q[0] = k[0, [TIES[t][0] for t in target]]
    s = (q[0] @ k[0, :TIE_N_KV].T) * _scale_log2(dtype)
    for i, t in enumerate(target):  # a check of the inputs: the tied keys lead every other key by >= 160 log2 units
        tied = np.zeros(TIE_N_KV, dtype=bool)
        tied[list(TIES[t])] = True
        assert (s[i, tied] == s[i].max()).all() and s[i].max() - s[i, ~tied].max() >= OH.MIN_GAP
    want = np.full(q.shape, RL.SENTINEL)
    want[0] = np.stack([v[0, list(TIES[t])].sum(0) / len(TIES[t]) for t in target])
    want = torch.as_tensor(want, dtype=torch.float64).to(dtype)
    qd, kd, vd = OH.tensors(dtype, dev(), q, k, v)
    out = torch.full(qd.shape, RL.SENTINEL, dtype=dtype, device=dev())
    ops.attn_fwd(qd, kd, vd, out, n_q=TIE_S, n_kv=TIE_N_KV, scale=OH.SCALE, n_splits=n_splits, variant=variant)
    torch.cuda.synchronize()
    got = out.cpu()
    bad = (got != want).any(-1).nonzero().tolist()
    assert torch.equal(got, want), f"{len(bad)} rows differ, first (head, row, tie) {[(h, r, TIES[target[r]]) for h, r in bad[:4]]}"
