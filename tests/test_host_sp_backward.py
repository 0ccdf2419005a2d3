"""CPU-only checks of the attention backward's algorithm under sequence parallelism: the `backward=` keyword of
`sp_soft_mixture_attention_autograd` (refused before any layout or collective), its way through the `routed` wrapper, and the
receive layout's address map that the deterministic passes rely on (tests/_sp_backward_workers.py `layout_precondition`, which
the GPU tests run on recorded launches, here on row maps alone)."""
import pytest
import torch

import _sp_backward_workers as W


class _Untouchable:
    """stands in for SP_STATE: any read of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"SP_STATE.{name} was read before the algorithm's name was checked")


def _tensors():
    q, k, v = (torch.zeros((1, 4, 16, 128), dtype=torch.bfloat16) for _ in range(3))
    return q, k, v, torch.zeros((1, 4, 3), dtype=torch.bfloat16)


def test_unknown_algorithm_is_refused_before_any_layout(monkeypatch):
    import vorta_amd.attention._sp as sp
    from vorta_amd import routed

    def untouchable(*a, **kw):
        raise AssertionError("a layout was built before the algorithm's name was checked")

    monkeypatch.setattr(sp, "SP_STATE", _Untouchable())
    for name in ("_mixture_setup", "_layout_only", "_layout", "UlyssesLayout", "geometry_for"):
        monkeypatch.setattr(sp, name, untouchable)
    q, k, v, sc = _tensors()
    for fn in (sp.sp_soft_mixture_attention_autograd, routed.sp_soft_mixture_attention_autograd):
        with pytest.raises(ValueError) as err:
            fn(q, k, v, 0, sc, model="wan", backward="nope")
        for algorithm in ("query_major", "key_major", "deterministic"):
            assert algorithm in str(err.value)
    # the process-wide routes are checked at the same place
    monkeypatch.setattr(routed, "_attention_backward", None)
    monkeypatch.setenv("VORTA_ATTENTION_BACKWARD", "fastest")
    with pytest.raises(ValueError):
        sp.sp_soft_mixture_attention_autograd(q, k, v, 0, sc, model="wan")


def test_routed_wrapper_forwards_the_keyword(monkeypatch):
    import vorta_amd.attention._sp as sp
    from vorta_amd import routed
    seen = {}
    monkeypatch.setattr(sp, "sp_soft_mixture_attention_autograd", lambda *a, **kw: seen.update(kw) or "out")
    q, k, v, sc = _tensors()
    assert routed.sp_soft_mixture_attention_autograd(q, k, v, 0, sc, model="wan", backward="key_major") == "out"
    assert seen == dict(model="wan", backward="key_major")


def test_valid_names_pass_the_check_and_reach_the_layout(monkeypatch):
    """a known name goes on to build the layout (here: a stub that ends the call), with the keyword or the switch"""
    import vorta_amd.attention._sp as sp
    from vorta_amd import routed

    class Reached(Exception):
        pass

    def setup(*a, **kw):
        raise Reached

    monkeypatch.setattr(sp, "_mixture_setup", setup)
    monkeypatch.setattr(routed, "_attention_backward", None)
    monkeypatch.delenv("VORTA_ATTENTION_BACKWARD", raising=False)
    q, k, v, sc = _tensors()
    for name in routed.ATTENTION_BACKWARDS + (None,):
        with pytest.raises(Reached):
            sp.sp_soft_mixture_attention_autograd(q, k, v, 0, sc, model="wan", backward=name)


def test_recv_function_takes_the_algorithm():
    """`_RecvSoftMixture.forward` has the algorithm as its last input (None: the process-wide choice)"""
    import inspect

    import vorta_amd.attention._sp as sp
    params = list(inspect.signature(sp._RecvSoftMixture.forward).parameters)
    assert params[-1] == "backward" and len(params) == 12  # ctx + 10 inputs + the algorithm


@pytest.mark.parametrize("S,T,P,Hl", [(576, 8, 2, 2), (576, 8, 2, 1), (576, 8, 4, 1), (576, 0, 2, 2), (576, 144, 4, 1),
                                      (118800, 256, 8, 3)])
def test_row_map_and_head_stride_address_every_row_once(S, T, P, Hl):
    """head * (S/P) + row_map[token] is one-to-one over (head slot, token) and stays inside the (P + 1) Hl S/P rows of a
    receive buffer -- the head views overlap, the addresses a kernel forms through them do not; the text segment included"""
    from vorta_amd.ulysses.engine import make_row_map
    Sl = S // P
    rm = make_row_map(S, T, P, Hl, "cpu").long()
    rows_total = (P + 1) * Hl * Sl
    view = ((Hl, rows_total - (Hl - 1) * Sl, 128), (Sl * 128, 128, 1))  # UlyssesLayout.head_view of a (rows_total, 128) buffer
    heads = torch.arange(Hl)
    one_to_one, inside = W._one_to_one(heads, rm[None].expand(Hl, S + T), *view)
    assert one_to_one and inside
    addr = heads[:, None] * Sl + rm[None]
    assert int(addr.max()) < rows_total
    # and what breaks it: a head stride one row short makes two (head, token) pairs meet
    if Hl > 1:
        bad = ((view[0]), ((Sl - 1) * 128, 128, 1))
        assert not W._one_to_one(heads, rm[None].expand(Hl, S + T), *bad)[0]


def test_layout_precondition_sees_a_repeated_row_and_a_repeated_head():
    """the host-side check the GPU tests rely on is not vacuous: a key list with a repeated row, a head list that names a head
    twice and two slots that meet in one accumulator row are each reported"""
    Sl, Hl, D = 16, 2, 128
    view = ((Hl, 3 * Hl * Sl - (Hl - 1) * Sl, D), (Sl * D, D, 1))
    acc = dict(dq=view, dk=view, dv=view)
    q = torch.empty((Hl, 1, D))
    rows = torch.arange(8, dtype=torch.int32)
    good = dict(q=q, n_q=8, n_kv=8, q_rows=rows, kv_rows=rows, tag="full")
    res = W.layout_precondition([good], acc)
    assert res["rows_distinct"] and res["heads_distinct"] and res["dq_one_to_one"] and res["dkv_one_to_one"] and res["inside"]
    repeated = torch.tensor([0, 1, 2, 3, 4, 5, 6, 6], dtype=torch.int32)
    res = W.layout_precondition([dict(good, kv_rows=repeated)], acc)
    assert not res["rows_distinct"] and not res["dkv_one_to_one"] and res["dq_one_to_one"]
    res = W.layout_precondition([dict(good, head_list=torch.tensor([1, 1], dtype=torch.int32))], acc)
    assert not res["heads_distinct"] and not res["dq_one_to_one"]
    # slot 0's row Sl is slot 1's row 0: distinct rows per slot, one address
    per_slot = torch.tensor([[Sl, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7]], dtype=torch.int32)
    res = W.layout_precondition([dict(good, kv_rows=per_slot)], acc)
    assert res["rows_distinct"] and not res["dkv_one_to_one"]
    res = W.layout_precondition([dict(good, q_rows=torch.arange(8, dtype=torch.int32) + view[0][1])], acc)
    assert not res["inside"]
