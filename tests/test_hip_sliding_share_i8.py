"""GPU: sliding_keys="share" under the int8-score precision "i8pv" (DESIGN.md 6.12, int8 scores).  `routed_attention` on the
local + white-noise head pair and the 16-tile geometry of tests/test_hip_sliding_share.py: the video rows of every (slot, tile)
bit for bit against an int8 table launch over the list the device chose (read back; the operands of `prepare_operands`), the
text-query rows (hunyuan) bit for bit against the same call under "window"; and the refusals that remain, by name."""
import pytest
import torch

import _structured_inputs as SI
import test_hip_attention_bwd as B
from _util import dev
from test_hip_sliding_content import _geom, _routed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", ["wan", "hunyuan"])
def test_share_under_i8pv_equals_table_launches_over_the_chosen_lists(model, golden):
    from vorta_amd import ops
    from vorta_amd.routed import prepare_operands
    _, t, te, q, k, v, _, _ = B._mixture_case(model, torch.bfloat16, golden, H=2)
    assert model == "wan" or t > te > 0
    gen = torch.Generator(device="cpu").manual_seed(5)
    local = SI.local_head(B.LATENT, (2.0, 3.0, 4.0), 8.0, 0.2, gen, "cpu")
    white = tuple(torch.randn((B.S_VID, 128), generator=gen) for _ in range(3))
    for x, a, b in zip((q, k, v), local, white):
        x[0, :, :B.S_VID] = torch.stack([a, b]).to(x.dtype).to(dev())
    geom = _geom(sliding_keys="share", mass_share=0.9)
    out = torch.full_like(q, 7.0)
    _routed(q, k, v, geom, model, t, te, out=out, fp8="i8pv")
    torch.cuda.synchronize()
    tabs, q_rows = geom.share_buffers(te, 2, 256), geom.sta_tables(te)[0]
    n_sel, count, kv_len = tabs.sel_tiles.shape[2], tabs.sel_count.cpu(), tabs.kv_len.cpu()
    print(f"kept tiles per head: mean {count.float().mean(1).tolist()}, min {int(count.min())}, max {int(count.max())} of {n_sel}")
    assert int(count.min()) < n_sel and int(count.max()) == n_sel, "the variable path needs short AND full lists"
    assert torch.equal(kv_len, count * geom.tok + te)
    kw = prepare_operands("i8pv", q[0], k[0], v[0], None).kwargs(None)
    for y in range(2):
        for i in range(kv_len.shape[1]):
            n, rows = int(kv_len[y, i]), q_rows[i * geom.tok:(i + 1) * geom.tok]
            alone = torch.full_like(q[0], 7.0)
            ops.attn_fwd(**kw, out=alone, n_q=geom.tok, q_rows=rows, n_kv=n, kv_rows=tabs.kv_rows[y, i, :n].contiguous(),
                         head_list=torch.tensor([y], dtype=torch.int32, device=dev()), n_heads=1, block_rows=256)
            assert torch.equal(out[0, y, rows.long()], alone[y, rows.long()]), (y, i, n)
    if t > 0:
        window = _routed(q, k, v, _geom(), model, t, te, fp8="i8pv")
        assert torch.equal(out[0, :, B.S_VID:], window[0, :, B.S_VID:])


def test_what_share_and_the_variable_length_launch_still_refuse(golden):
    from vorta_amd import _C, ops
    _, t, te, q, k, v, _, _ = B._mixture_case("wan", torch.bfloat16, golden, H=2)
    geom = _geom(sliding_keys="share", mass_share=0.9)
    for precision, missing in (("fp8pv", "no mixed-precision one"), ("auto8", "which 'auto8' needs")):
        with pytest.raises(ValueError, match=f"sliding_keys='share' under precision '{precision}'.*{missing}"):
            _routed(q, k, v, geom, "wan", t, te, fp8=precision)
    q3, k3, v3 = q[0], k[0], v[0]
    v8, vd, _ = ops.fp8_quantize_v(v3)
    i8 = ops.i8_quantize_k(q3, k3)
    f8 = ops.fp8_quantize_qkv(q3, k3, v3)
    n = 64
    rows = torch.arange(n, dtype=torch.int32, device=dev())
    kw = dict(kv_len=torch.full((2, 1), n, dtype=torch.int32, device=dev()), n_q=n, n_kv=n, kv_rows=rows, out=torch.empty_like(q3))
    with pytest.raises(ValueError, match=r"no mixed-precision \(16-bit k, e4m3 v\) variable-length body"):
        ops.attn_fwd_varlen(q3, k3, v8, v_descale=vd, **kw)
    with pytest.raises(ValueError, match=r"no all-e4m3 \(e4m3 q, k\) variable-length body"):
        ops.attn_fwd_varlen(f8.q, f8.k, f8.v, v_descale=f8.v_descale, **kw)
    dup = torch.full((n, 1), n, dtype=torch.int32, device=dev())
    for bad in (dict(n_splits=2), dict(dup_rows=dup)):
        with pytest.raises(_C.VortaHipError, match="VORTA_EUNSUPPORTED"):
            ops.attn_fwd_varlen(q3, i8.k8, v8, v_descale=vd, i8=i8, **kw, **bad)
