"""A plain torch restatement of ONE ops.attn_fwd launch, differentiable, in any dtype (tests/test_hip_attention_bwd.py):
gather the rows the launch names, softmax(q k^T * scale) v, zero rows past the effective q_valid, copy duplicates.  It reads
the same keyword dictionary the launcher takes -- head lists and device head counts, query groups of equal or different
lengths, row tables, duplicate rows, host and device lengths -- and nothing of the library."""
import math

import torch


def _cpu(t):
    return None if t is None else t.detach().cpu().long()


def launch_geometry(kw, n_heads_buf):
    """(heads, groups, n_kv_eff, q_valid_eff) of a launch: live head per slot, (group, first, end) query segments"""
    hl = _cpu(kw.get("head_list"))
    n_heads = kw.get("n_heads")
    if n_heads is None:
        n_heads = len(hl) if hl is not None else n_heads_buf
    heads = (hl[:n_heads] if hl is not None else torch.arange(n_heads)).tolist()
    if kw.get("n_heads_dev") is not None:
        heads = heads[: max(int(kw["n_heads_dev"].item()), 0)]
    n_q, n_kv = kw["n_q"], kw["n_kv"]
    q_valid = n_q if kw.get("q_valid") is None else kw["q_valid"]
    if kw.get("n_kv_dev") is not None:
        n_kv = max(1, min(int(kw["n_kv_dev"].item()), n_kv))
    if kw.get("q_valid_dev") is not None:
        q_valid = min(int(kw["q_valid_dev"].item()), q_valid)
    if kw.get("q_block_table") is not None:
        groups = [tuple(r) for r in _cpu(kw["q_block_table"]).tolist()]
    else:
        glen = kw.get("q_group_len", 0) or n_q
        groups = [(g, g * glen, min((g + 1) * glen, n_q)) for g in range(-(-n_q // glen))]
    return heads, groups, n_kv, q_valid


def restate(kw, q, k, v, out):
    """write the launch's output rows into `out` ((H,S,D), modified in place, autograd-tracked) and return it"""
    heads, groups, n_kv, q_valid = launch_geometry(kw, q.shape[0])
    scale = kw.get("scale") or 1.0 / math.sqrt(q.shape[-1])
    q_rows, kv_rows, dup = _cpu(kw.get("q_rows")), _cpu(kw.get("kv_rows")), _cpu(kw.get("dup_rows"))
    sg = kw.get("kv_rows_stride_g", 0)
    for y, h in enumerate(heads):
        if q_rows is None:
            qr = torch.arange(kw.get("q_row_offset", 0), kw.get("q_row_offset", 0) + kw["n_q"])
        else:
            qr = q_rows[y] if q_rows.dim() == 2 else q_rows
        for g, a, b in groups:
            if b <= a:
                continue
            pos = torch.arange(a, b)
            rows = qr[pos].to(q.device)
            if kv_rows is None:
                keys = torch.arange(kw.get("kv_row_offset", 0), kw.get("kv_row_offset", 0) + n_kv)
            elif sg > 0:
                keys = kv_rows.reshape(-1)[g * sg: g * sg + n_kv]
            else:
                keys = (kv_rows[y] if kv_rows.dim() == 2 else kv_rows)[:n_kv]
            keys = keys.to(q.device)
            p = torch.softmax((q[h, rows] @ k[h, keys].transpose(0, 1)) * scale, dim=-1)
            o = p @ v[h, keys]
            o = torch.where((pos < q_valid).to(q.device)[:, None], o, torch.zeros_like(o))
            out[h, rows] = o
        if dup is not None:
            dr = dup[y] if dup.dim() == 3 else dup
            npos = kw.get("n_dup_pos", 0) or dr.shape[0]
            if npos:
                src = out[h, qr[:npos].to(q.device)]
                out[h, dr[:npos].reshape(-1).to(q.device)] = src.repeat_interleave(dr.shape[1], dim=0)
    return out


def named_rows(kw, shape):
    """boolean (H,S) masks of the rows a launch may give a gradient: (query rows at positions below the effective q_valid,
    key rows below the effective n_kv of any group) of the live heads -- every other row must receive exactly zero"""
    heads, groups, n_kv, q_valid = launch_geometry(kw, shape[0])
    qm, km = torch.zeros(shape[:2], dtype=torch.bool), torch.zeros(shape[:2], dtype=torch.bool)
    q_rows, kv_rows = _cpu(kw.get("q_rows")), _cpu(kw.get("kv_rows"))
    sg = kw.get("kv_rows_stride_g", 0)
    for y, h in enumerate(heads):
        if q_rows is None:
            qr = torch.arange(kw.get("q_row_offset", 0), kw.get("q_row_offset", 0) + kw["n_q"])
        else:
            qr = q_rows[y] if q_rows.dim() == 2 else q_rows
        for g, a, b in groups:
            if b <= a:
                continue
            qm[h, qr[a:min(b, q_valid)]] = True
            if kv_rows is None:
                keys = torch.arange(kw.get("kv_row_offset", 0), kw.get("kv_row_offset", 0) + n_kv)
            elif sg > 0:
                keys = kv_rows.reshape(-1)[g * sg: g * sg + n_kv]
            else:
                keys = (kv_rows[y] if kv_rows.dim() == 2 else kv_rows)[:n_kv]
            km[h, keys] = True
    return qm, km
