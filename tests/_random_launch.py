"""Random launch geometry for the attention kernels of every family (tests/test_hip_attention.py,
tests/test_hip_attention_random.py): head lists and device head counts, query groups of equal or different lengths
(q_block_table) with their own key lists, row tables, duplicate rows, q_valid / n_kv tails on the host and on the device,
key splits and workgroup sizes.  Every table entry is in range, so a wrong kernel writes wrong values but stays inside its
buffers."""
from types import SimpleNamespace

import numpy as np
import torch

SENTINEL = 7.0  # every row a launch does not name keeps it


def draw(rng, *, S_range=(64, 700), H_max=4, max_splits=8, block_rows=None, device_lengths=True, heads_dev=True,
         H_buf=None, S=None, empty_tail=False):
    """one random launch over (H_buf, S, 128) buffers (drawn unless given); `block_rows` fixes the workgroup size (else
    0, 128 or 256); `empty_tail`: key splits and a device n_kv that leaves the last split(s) without keys"""
    H_buf = int(rng.integers(1, H_max + 1)) if H_buf is None else H_buf
    S = int(rng.integers(*S_range)) if S is None else S
    heads = rng.permutation(H_buf)[: int(rng.integers(1, H_buf + 1))].astype(np.int32)
    n_heads_dev = int(rng.integers(0, len(heads) + 1)) if heads_dev and rng.integers(0, 3) == 0 else None
    br = int(rng.choice([0, 128, 256])) if block_rows is None else block_rows
    mode = ("one", "equal", "table")[int(rng.integers(0, 3))]
    if mode == "table" and br == 0:
        br = int(rng.choice([128, 256]))  # a q_block_table names its workgroup size
    use_qtab = mode != "one" or bool(rng.integers(0, 2))
    qtab = None
    if mode == "one":
        n_q = int(rng.integers(1, S + 1))
        bounds = [(0, n_q)]
        glen = 0
    elif mode == "equal":
        n_groups = int(rng.integers(1, 5))
        glen = int(rng.integers(1, max(2, S // n_groups)))
        n_q = n_groups * glen - int(rng.integers(0, glen))  # the last group may be short
        bounds = [(g * glen, min((g + 1) * glen, n_q)) for g in range(-(-n_q // glen))]
    else:  # groups of different lengths, each cut into workgroups of br rows from its start
        n_groups = int(rng.integers(1, 5))
        cuts = np.sort(rng.choice(np.arange(1, S), size=n_groups, replace=False))
        n_q = int(cuts[-1])
        edges = [0] + cuts.tolist()
        bounds = [(edges[g], edges[g + 1]) for g in range(n_groups)]
        glen = 0
        qtab = np.array([(g, p, min(p + br, b)) for g, (a, b) in enumerate(bounds) for p in range(a, b, br)], dtype=np.int32)
    n_groups = len(bounds)
    n_kv = int(rng.integers(min(129, S) if empty_tail else 1, S + 1))
    q_rows = rng.permutation(S)[:n_q].astype(np.int32) if use_qtab else None
    q_off = 0 if use_qtab else int(rng.integers(0, S - n_q + 1))
    per_group = n_groups > 1 or mode != "one"
    use_kvtab = per_group or bool(rng.integers(0, 2))
    kv_rows = np.stack([rng.permutation(S)[:n_kv] for _ in range(n_groups)]).astype(np.int32) if use_kvtab else None
    kv_off = 0 if use_kvtab else int(rng.integers(0, S - n_kv + 1))
    q_valid = int(rng.integers(0, n_q + 1)) if rng.integers(0, 3) == 0 else n_q
    n_splits = int(rng.integers(2 if empty_tail else 1, max_splits + 1)) if empty_tail or rng.integers(0, 2) else 1
    written = q_rows if use_qtab else np.arange(q_off, q_off + n_q, dtype=np.int32)
    rest = np.setdiff1d(np.arange(S), written)
    dup, n_dup_pos = None, 0
    if len(rest) >= 2 and rng.integers(0, 2):
        n_dup = int(rng.integers(1, 3))
        n_dup_pos = int(rng.integers(1, min(n_q, len(rest) // n_dup) + 1))
        dup = rng.permutation(rest)[: n_dup_pos * n_dup].reshape(n_dup_pos, n_dup).astype(np.int32)
    # device-resident lengths (vorta_attn_args.n_kv_dev / q_valid_dev): effective n_kv = clamp(*n_kv_dev, 1, n_kv),
    # effective q_valid = min(*q_valid_dev, q_valid)
    n_kv_dev = q_valid_dev = None
    if device_lengths and (empty_tail or rng.integers(0, 3)):
        nblk = -(-n_kv // 64)
        bps = -(-nblk // n_splits)
        kinds = ("below", "equal", "above", "zero") + ("empty tail",) * (3 if n_splits > 1 else 0)
        kind = "empty tail" if empty_tail else kinds[int(rng.integers(0, len(kinds)))]
        if kind == "empty tail" and n_splits > 1 and nblk > 1:
            # the last j splits start at or past the effective end: their partials are m = -1e30, l = 0.  Fewer splits
            # first if the host n_kv already leaves the last one empty (ceil(nblk / n_splits) blocks per split)
            while n_splits > 2 and (n_splits - 1) * bps >= nblk:
                n_splits -= 1
                bps = -(-nblk // n_splits)
            j = int(rng.integers(1, n_splits))
            n_kv_dev = int(rng.integers(1, min(n_kv, max(1, (n_splits - j) * bps * 64)) + 1))
        elif kind == "below" and n_kv > 1:
            n_kv_dev = int(rng.integers(1, n_kv))
        elif kind == "above":
            n_kv_dev = n_kv + int(rng.integers(1, 200))
        elif kind == "zero":
            n_kv_dev = 0
        else:
            n_kv_dev = n_kv
    if device_lengths and rng.integers(0, 3):
        kind = int(rng.integers(0, 3))
        q_valid_dev = 0 if kind == 0 else int(rng.integers(0, q_valid + 1)) if kind == 1 else q_valid + int(rng.integers(1, 100))
    L = SimpleNamespace(H_buf=H_buf, S=S, heads=heads, n_heads_dev=n_heads_dev, block_rows=br, mode=mode, glen=glen,
                        bounds=bounds, qtab=qtab, n_q=n_q, q_rows=q_rows, q_off=q_off, kv_rows=kv_rows, kv_off=kv_off,
                        per_group=per_group, n_kv=n_kv, q_valid=q_valid, n_splits=n_splits, dup=dup, n_dup_pos=n_dup_pos,
                        n_kv_dev=n_kv_dev, q_valid_dev=q_valid_dev, written=written)
    L.n_kv_eff = n_kv if n_kv_dev is None else max(1, min(n_kv_dev, n_kv))
    L.q_valid_eff = q_valid if q_valid_dev is None else min(q_valid_dev, q_valid)
    L.live = heads if n_heads_dev is None else heads[:n_heads_dev]
    return L


def kwargs(L, dev, **over):
    """ops.attn_fwd keywords of launch L (device tables on `dev`); `over` replaces any of them"""
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev)  # noqa: E731
    kv = L.kv_rows if (L.kv_rows is None or L.per_group) else L.kv_rows[0]  # 1-D = one list shared by all heads
    kw = dict(n_q=L.n_q, q_group_len=L.glen, n_kv=L.n_kv, q_valid=L.q_valid, head_list=t(L.heads), n_heads=len(L.heads),
              q_rows=t(L.q_rows), q_row_offset=L.q_off, kv_rows=t(kv), kv_row_offset=L.kv_off,
              kv_rows_stride_g=L.n_kv if L.per_group else 0, dup_rows=t(L.dup), n_dup_pos=L.n_dup_pos, n_splits=L.n_splits,
              block_rows=L.block_rows)
    if L.n_heads_dev is not None:
        kw["n_heads_dev"] = torch.tensor([L.n_heads_dev], dtype=torch.int32, device=dev)
    if L.n_kv_dev is not None:
        kw["n_kv_dev"] = torch.tensor([L.n_kv_dev], dtype=torch.int32, device=dev)
    if L.q_valid_dev is not None:
        kw["q_valid_dev"] = torch.tensor([L.q_valid_dev], dtype=torch.int32, device=dev)
    if L.qtab is not None:
        kw.update(q_block_table=t(L.qtab), n_key_lists=len(L.bounds))
    kw.update(over)
    return kw


def emulator_kwargs(L):
    """O.fp8_attn_launch keywords of launch L for one head: the effective lengths, the split boundaries of the host n_kv"""
    kv = L.kv_rows if (L.kv_rows is None or L.per_group) else L.kv_rows[0]
    return dict(n_q=L.n_q, n_kv=L.n_kv_eff, split_n_kv=L.n_kv, q_rows=L.q_rows, q_row_offset=L.q_off, q_valid=L.q_valid_eff,
                kv_rows=kv, kv_row_offset=L.kv_off, dup_rows=L.dup, n_dup_pos=L.n_dup_pos, n_splits=L.n_splits,
                q_group_bounds=L.bounds)


def dense_reference(L, q, k, v, attend):
    """(H_buf, S, 128) float64 expected output of launch L: attend(q_rows, k_rows, v_rows) per live head and group over the
    effective keys, zeros past the effective q_valid, duplicates copied, SENTINEL elsewhere"""
    ref = np.full((L.H_buf, L.S, q.shape[-1]), SENTINEL)
    for h in L.live:
        for g, (a, b) in enumerate(L.bounds):
            pos = np.arange(a, b)
            rows = L.written[pos]
            keys = L.kv_rows[g if L.per_group else 0] if L.kv_rows is not None else np.arange(L.kv_off, L.kv_off + L.n_kv)
            keys = keys[:L.n_kv_eff]
            o = attend(q[h, rows], k[h, keys], v[h, keys])
            o[pos >= L.q_valid_eff] = 0.0
            ref[h, rows] = o
        for p in range(L.n_dup_pos):
            ref[h, L.dup[p]] = ref[h, L.written[p]]
    return ref


def describe(L):
    return dict(H_buf=L.H_buf, S=L.S, heads=L.heads.tolist(), n_heads_dev=L.n_heads_dev, mode=L.mode, bounds=L.bounds,
                n_kv=L.n_kv, n_kv_dev=L.n_kv_dev, q_valid=L.q_valid, q_valid_dev=L.q_valid_dev, n_splits=L.n_splits,
                block_rows=L.block_rows, qtab=L.q_rows is not None, kvtab=L.kv_rows is not None, n_dup_pos=L.n_dup_pos)
