"""GPU parity of the 16-bit pipelined attention loop at the ends of a key range: key counts around every 64-key block
boundary and around the point where the loop leaves its clamp-free main part, through the dense body and through a
key table, at both workgroup sizes, with split keys, a device-resident key count and one fused grid -- against the
float64 oracle.

Every K/V row the launch must not use (rows outside [kv_row_offset, kv_row_offset + n_kv), rows no table entry names,
the padding columns of a padded buffer) holds NaN, and so does every row a stray table entry could name (the 64 table
entries behind each key list name such a row).  What that sentinel can and cannot show:
  * a stray V row shows: its probability is 0 and 0 x NaN = NaN reaches the output;
  * a stray K row of a partial block does NOT show: its score is masked to -inf before anything reads it (and such a
    row is harmless for the same reason); a stray K row inside a whole block would show, as a NaN score;
  * a dense request past the END of the buffers shows only as far as NaN rows follow (`after` rows); with after = 0 the
    allocation ends with the last key, but the allocator rounds a block up to 512 bytes and hands out parts of larger
    ones, so one row too far neither faults nor reads NaN there: that case checks values at an exact extent, it does
    not prove the absence of such a read."""
import numpy as np
import pytest
import torch

from oracle import vorta_oracle as O

pytestmark = pytest.mark.gpu

from _util import check, dev, rounded  # noqa: E402

H, D = 2, 128
# One block is 64 keys.  The clamp-free main loop runs pairs of steps j < n_kv/64 - 2 (dense: a step requests tiles two
# blocks ahead) or j < n_kv/64 - 3 (key table: it also loads the row ids of the block after those), so its first pair
# runs from 256 keys on (dense) and from 320 on (table), its second from 384 / 448.
N_KV = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]  # every block boundary; 257 enters the dense main loop
N_KV_DENSE = N_KV + [255, 256, 321, 385]                     # around the dense main loop's first and second pair
N_KV_TABLE = N_KV + [319, 320, 321, 383, 384, 385, 449]      # around the table main loop's first and second pair
N_Q = [1, 33, 256, 257]  # an inactive wave, a partial wave, one full workgroup, two workgroups
DTYPES = [torch.bfloat16, torch.float16]
_RNG = np.random.default_rng(20)
_Q = _RNG.standard_normal((H, 600, D))
N_ROWS, N_USABLE = 520, 480  # rows of the K/V buffers behind a key table; the rows from N_USABLE on hold NaN
_K = _RNG.standard_normal((H, N_ROWS, D))
_V = _RNG.standard_normal((H, N_ROWS, D))


def _dev16(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dtype).to(dev())


def _kv_views(layout, dtype, n_valid, off, after):
    """K, V as (H, off + n_valid + after, D) device views; rows [off, off + n_valid) hold _K / _V, all else is NaN.
    'padded': rows of 192 (K) and 256 (V) elements, so the two row strides differ; 'proj': heads of one (S, H*D)
    buffer each, both row strides H*D; with after = 0 the last row of the last head ends the allocation."""
    R = off + n_valid + after
    views = []
    for src, width in ((_K, 192), (_V, 256)):
        if layout == "padded":
            buf = torch.full((H, R, width), float("nan"), dtype=dtype, device=dev())
            view = buf[:, :, :D]
        else:
            buf = torch.full((R, H * D), float("nan"), dtype=dtype, device=dev())
            view = buf.view(R, H, D).permute(1, 0, 2)
        view[:, off:off + n_valid] = _dev16(src[:, :n_valid], dtype)
        views.append(view)
    return views


def _dense_case(dtype, n_q, n_kv, layout="padded", off=5, after=3, **kw):
    from vorta_amd import ops
    kd, vd = _kv_views(layout, dtype, kw.pop("n_valid", n_kv), off, after)
    qd = _dev16(_Q[:, :n_q], dtype)
    out = torch.full((H, n_q + 2, D), 7.0, dtype=dtype, device=dev())
    ops.attn_fwd(qd, kd, vd, out, n_q=n_q, n_kv=n_kv, kv_row_offset=off, **kw)
    return out


def _dense_ref(dtype, n_q, n_valid):
    return O.dense_attention(rounded(_Q[:, :n_q], dtype), rounded(_K[:, :n_valid], dtype), rounded(_V[:, :n_valid], dtype))


def _verify(out, ref, dtype, n_q, what, failures):
    """values against the oracle (NaN fails the comparison), rows behind n_q untouched"""
    try:
        assert not torch.isnan(out[:, :n_q]).any(), "NaN in the output"
        check(out[:, :n_q], ref, dtype)
        assert torch.all(out[:, n_q:] == 7.0), "rows behind n_q were written"
    except AssertionError as e:
        failures.append(f"{what}: {e}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("n_q", N_Q)
def test_dense_key_counts_around_block_boundaries(dtype, block_rows, n_q):
    """dense body of either workgroup size, K and V in differently padded buffers (k_ss != v_ss), kv_row_offset != 0"""
    failures = []
    for n_kv in N_KV_DENSE:
        out = _dense_case(dtype, n_q, n_kv, block_rows=block_rows)
        _verify(out, _dense_ref(dtype, n_q, n_kv), dtype, n_q, f"n_kv={n_kv}", failures)
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("after", [0, 4])
def test_dense_heads_of_one_projection_buffer(dtype, block_rows, after):
    """k_ss == v_ss == H*D; after = 0: the allocation holds exactly the rows up to the last key, so a request one row
    too far leaves the tensor; after = 4: NaN rows follow it"""
    failures = []
    for n_kv in N_KV:
        out = _dense_case(dtype, 33, n_kv, layout="proj", off=64 if n_kv % 2 else 0, after=after, block_rows=block_rows)
        _verify(out, _dense_ref(dtype, 33, n_kv), dtype, 33, f"n_kv={n_kv}", failures)
    assert not failures, failures


def _table(n_kv, rng, n_rows=N_ROWS, n_usable=N_USABLE, gap=64, guard=256):
    """two key lists (one per query group) of n_kv distinct rows out of the first n_usable; every other entry of the
    table buffer (a whole block of them directly behind each list, more at the end) names a NaN row"""
    stride_g = n_kv + gap
    tab = np.full(2 * stride_g + guard, n_rows - 1, np.int32)
    lists = [rng.permutation(n_usable)[:n_kv].astype(np.int32) for _ in range(2)]
    for g in range(2):
        tab[g * stride_g:g * stride_g + n_kv] = lists[g]
    return tab, lists, stride_g


def _table_case(dtype, glen, n_kv, rng, **kw):
    from vorta_amd import ops
    tab, lists, stride_g = _table(kw.pop("n_valid", n_kv), rng)
    kd, vd = _kv_views("padded", dtype, N_USABLE, 0, N_ROWS - N_USABLE)
    n_q = 2 * glen
    qd = _dev16(_Q[:, :n_q], dtype)
    out = torch.full((H, n_q + 2, D), 7.0, dtype=dtype, device=dev())
    ops.attn_fwd(qd, kd, vd, out, n_q=n_q, q_group_len=glen, n_kv=n_kv, kv_rows=torch.as_tensor(tab, device=dev()),
                 kv_rows_stride_g=stride_g, **kw)
    rq, rk, rv = rounded(_Q[:, :n_q], dtype), rounded(_K, dtype), rounded(_V, dtype)
    ref = np.concatenate([O.dense_attention(rq[:, g * glen:(g + 1) * glen], rk[:, lists[g]], rv[:, lists[g]])
                          for g in range(2)], axis=1)
    return out, ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block_rows", [128, 256])
@pytest.mark.parametrize("glen", [33, 257])
def test_key_table_counts_around_block_boundaries(dtype, block_rows, glen):
    """the same key counts, and those around the table body's own main loop, through a permuted key table with one
    list per query group, in the table body of either workgroup size"""
    rng = np.random.default_rng(21)
    failures = []
    for n_kv in N_KV_TABLE:
        out, ref = _table_case(dtype, glen, n_kv, rng, block_rows=block_rows)
        _verify(out, ref, dtype, 2 * glen, f"n_kv={n_kv}", failures)
    assert not failures, failures


@pytest.mark.parametrize("n_splits", [2, 3])
@pytest.mark.parametrize("n_kv", [200, 321])
def test_split_keys_end_in_partial_and_full_blocks(n_splits, n_kv):
    """200 keys = 3 blocks + 8 keys, 321 = 5 blocks + 1: with 2 or 3 splits one split ends in the partial block, the
    others in whole ones (and 200 keys in 3 splits leave the last split empty)"""
    dtype = torch.float16
    rng = np.random.default_rng(22)
    failures = []
    out = _dense_case(dtype, 257, n_kv, n_splits=n_splits)
    _verify(out, _dense_ref(dtype, 257, n_kv), dtype, 257, "dense", failures)
    out, ref = _table_case(dtype, 33, n_kv, rng, n_splits=n_splits)
    _verify(out, ref, dtype, 66, "table", failures)
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_key_count_below_the_host_bound(dtype):
    """n_kv = 256 on the host, 130 on the device: the loop's parts and the tail mask follow the device value (rows
    130 ... 255 hold NaN)"""
    rng = np.random.default_rng(23)
    n_dev = torch.tensor([130], dtype=torch.int32, device=dev())
    failures = []
    out = _dense_case(dtype, 257, 256, n_valid=130, after=126 + 3, n_kv_dev=n_dev)
    _verify(out, _dense_ref(dtype, 257, 130), dtype, 257, "dense", failures)
    out, ref = _table_case(dtype, 33, 256, rng, n_valid=130, n_kv_dev=n_dev)
    _verify(out, ref, dtype, 66, "table", failures)
    assert not failures, failures


def test_fused_grid_dense_table_and_grouped_table():
    """vorta_attn_fwd_batch: four segments of one grid, each with an odd key count; the last one (a grouped table of
    321 keys) runs the table body's main loop inside the fused kernel"""
    from vorta_amd import ops
    dtype = torch.bfloat16
    rng = np.random.default_rng(24)
    S = 300
    kd, vd = _kv_views("padded", dtype, N_USABLE, 0, N_ROWS - N_USABLE)
    qd = _dev16(_Q[:, :S], dtype)
    rq, rk, rv = rounded(_Q[:, :S], dtype), rounded(_K, dtype), rounded(_V, dtype)
    outs = [torch.full((H, S + 2, D), 7.0, dtype=dtype, device=dev()) for _ in range(4)]
    one = np.full(171 + 256, N_ROWS - 1, np.int32)
    keys1 = rng.permutation(N_USABLE)[:171].astype(np.int32)
    one[:171] = keys1
    tabs = [_table(n_kv, rng) for n_kv in (77, 321)]
    grouped = [dict(q=qd, k=kd, v=vd, out=outs[2 + i], n_q=S, q_group_len=150, n_kv=n_kv,
                    kv_rows=torch.as_tensor(tab, device=dev()), kv_rows_stride_g=stride_g, block_rows=256)
               for i, (n_kv, (tab, _, stride_g)) in enumerate(zip((77, 321), tabs))]
    ops.attn_fwd_batch([
        dict(q=qd, k=kd, v=vd, out=outs[0], n_q=S, n_kv=299, kv_row_offset=7, block_rows=256),
        dict(q=qd, k=kd, v=vd, out=outs[1], n_q=S, n_kv=171, kv_rows=torch.as_tensor(one, device=dev()), block_rows=256),
        *grouped])
    refs = [O.dense_attention(rq, rk[:, 7:306], rv[:, 7:306]), O.dense_attention(rq, rk[:, keys1], rv[:, keys1])]
    for _, lists, _ in tabs:
        refs.append(np.concatenate([O.dense_attention(rq[:, g * 150:(g + 1) * 150], rk[:, lists[g]], rv[:, lists[g]])
                                    for g in range(2)], axis=1))
    failures = []
    for i in range(4):
        _verify(outs[i], refs[i], dtype, S, f"segment {i}", failures)
    assert not failures, failures
