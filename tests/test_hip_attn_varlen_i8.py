"""GPU: vorta_attn_fwd_varlen_i8 (csrc/attn_fwd_i8_varlen.hip) on hand-made tables.  Three head slots behind the head list
(2, 0, 1) with a device count of 2 (the third slot keeps its fill), seven query groups of 110 positions over a random q_rows;
per slot the groups attend a rotation of 1, 37, 128, 190, 256, 261, 530 = n_kv keys: 1, 1, 2, 3, 4, 5 and 9 key blocks, tails
of 1, 37, 0, 62, 0, 5, 18 -- every exit of the 4-way unrolled loop, two rounds of it, and lists shorter than the pipeline is
deep.  Every list entry behind a group's length names row S - 1, whose e4m3 V bytes are NaN and whose k_bias is 1e30.
(a) no NaN, untouched rows keep the fill; (b) every (slot, group) bit for bit against vorta_attn_fwd_i8 over that group's list
alone (same arithmetic by construction: margin zero); (c) against float64 softmax attention over exactly the listed keys on the
operands the kernel reads, rel_fro <= RELF_DIRECT per head (tests/test_hip_i8.py's bound for this comparison; the emulator
alone sits at <= 0.75 of it on these inputs: profiles/share_tiles_i8_accuracy.txt)."""
import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O

from _util import dev, rel_fro, to_dev
from test_hip_i8 import RELF_DIRECT, _hooks, _vdec

pytestmark = pytest.mark.gpu

H, S, GLEN, N_G, N_KV, FILL = 3, 800, 110, 7, 530, 7.0
N_Q = GLEN * N_G
HEADS, LIVE = [2, 0, 1], 2
LENS = [1, 37, 128, 190, 256, 261, 530]
_cases = {}


def _case(dtype):
    """operands, tables and the float64 reference of gate (c), once per dtype"""
    if dtype in _cases:
        return _cases[dtype]
    from vorta_amd import ops
    rng = np.random.default_rng(1)
    q = rng.standard_normal((H, S, 128)) + 0.8 * rng.standard_normal((H, 1, 128))
    k, v = rng.standard_normal((H, S, 128)) + 0.5, rng.standard_normal((H, S, 128))
    qd, kd = to_dev(q, dtype), to_dev(k, dtype)
    i8 = ops.i8_quantize_k(qd, kd)
    v8, vd, _ = ops.fp8_quantize_v(to_dev(v * np.linspace(0.05, 8.0, 128), dtype))
    v8[:, S - 1], i8.k_bias[:, S - 1] = 0x7F, 1e30
    q_rows = rng.permutation(S - 1)[:N_Q].astype(np.int32)
    kv_len = np.stack([np.roll(LENS, y) for y in range(H)]).astype(np.int32)
    kv_rows = np.full((H, N_G, N_KV), S - 1, np.int32)
    for y in range(H):
        for g in range(N_G):
            kv_rows[y, g, :kv_len[y, g]] = rng.permutation(S - 1)[:kv_len[y, g]]
    hooks, (ve, vde) = _hooks(qd, i8), _vdec(v8, vd)
    exact = np.zeros((H, S, 128))
    for y in range(LIVE):
        for g in range(N_G):
            n, h = int(kv_len[y, g]), HEADS[y]
            O.fp8_attn_launch(None, None, ve[h], exact[h], vde[h], n_q=GLEN, n_kv=n, q_rows=q_rows[g * GLEN:(g + 1) * GLEN],
                              kv_rows=kv_rows[y, g, :n], round_p=False, wave_operands=hooks[h])
    _cases[dtype] = qd, i8, v8, vd, q_rows, kv_rows, kv_len, exact
    return _cases[dtype]


@pytest.mark.parametrize("reverse", [False, True], ids=["index_order", "reversed_order"])
@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_int8_groups_of_different_key_counts_in_one_launch(dtype, block_rows, reverse):
    from vorta_amd import ops
    qd, i8, v8, vd, q_rows, kv_rows, kv_len, exact = _case(dtype)
    t = lambda a: torch.as_tensor(a, device=dev())  # noqa: E731
    out = torch.full_like(qd, FILL)
    kv, qr = t(kv_rows), t(q_rows)
    n_wg = H * N_G * -(-GLEN // block_rows)
    order = torch.arange(n_wg - 1, -1, -1, dtype=torch.int32, device=dev()) if reverse else None
    ops.attn_fwd_varlen(qd, i8.k8, v8, out, kv_len=t(kv_len), order=order, n_q=N_Q, q_group_len=GLEN, n_kv=N_KV, q_rows=qr,
                        kv_rows=kv, kv_rows_stride_g=kv.stride(1), head_list=t(np.array(HEADS, np.int32)), n_heads=H,
                        n_heads_dev=t(np.array([LIVE], np.int32)), block_rows=block_rows, v_descale=vd, i8=i8)
    torch.cuda.synchronize()
    # (a)
    assert not torch.isnan(out).any(), "a key behind a group's length was read"
    untouched = torch.ones(S, dtype=torch.bool, device=dev())
    untouched[qr.long()] = False
    assert (out[HEADS[LIVE]] == FILL).all() and (out[:, untouched] == FILL).all()
    # (b)
    for y in range(LIVE):
        for g in range(N_G):
            n, rows = int(kv_len[y, g]), qr[g * GLEN:(g + 1) * GLEN]
            alone = torch.full_like(qd, FILL)
            ops.attn_fwd(qd, i8.k8, v8, alone, n_q=GLEN, n_kv=n, q_rows=rows, kv_rows=kv[y, g, :n].contiguous(),
                         head_list=t(np.array([HEADS[y]], np.int32)), n_heads=1, block_rows=block_rows, v_descale=vd, i8=i8)
            assert torch.equal(out[HEADS[y], rows.long()], alone[HEADS[y], rows.long()]), (y, g, n)
    # (c)
    got = out.float().cpu().numpy()
    for y in range(LIVE):
        err = rel_fro(got[HEADS[y], q_rows], exact[HEADS[y], q_rows])
        print(f"slot {y}: rel_fro against float64 over the listed keys {err:.3e} (bound {RELF_DIRECT})")
        assert err <= RELF_DIRECT
