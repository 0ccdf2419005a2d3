"""The Ulysses exchange behind autograd (router training under sequence parallelism).

Autograd functions over the engine's own primitives (engine.py `UlyssesLayout.scatter_heads`, `gather_heads`,
`gather_heads_multi`): one `all_to_all_single` per tensor in either direction, no second transport.  Their derivatives are the
reference's (vorta/ulysses/utils.py:96-162):
  * the gradient of sequence shards -> head shards is head shards -> sequence shards, and the reverse (utils.py:111-120);
  * the gradient of the text all-gather is the rank's own head slice (utils.py:148-158): every rank sees the same loss on the
    replicated text rows, so nothing is summed;
  * the gradient of `shrink_dim` (a head's text rows are copied behind its video rows on the rank that owns it) is zero
    outside the rank's heads.
So a rank produces text-row gradients for its local heads only and zeros elsewhere; their sum over the ranks is the
single-process gradient.
Every call allocates its receive buffers: a tensor an autograd node keeps must outlive the next layer's exchange, which the
shared buffers of the inference path (attention/_sp.py `_BUFFERS`) do not.
"""
from typing import List, Sequence

import torch

from .engine import UlyssesLayout


def new_recv_buffer(lay: UlyssesLayout, dtype=None) -> torch.Tensor:
    """a receive buffer of this call's own: the exchange writes every video row, the rows behind them are zeroed (a head's
    segment there holds its T text rows and Sl - T rows nothing writes)"""
    buf = torch.empty((lay.rows_total, lay.D), dtype=lay.dtype if dtype is None else dtype, device=lay.device)
    buf[lay.rows_video:].zero_()
    return buf


def _text_view(lay: UlyssesLayout, buf: torch.Tensor) -> torch.Tensor:
    return lay.grouping(1)[0][0].text_view(buf)


class _ScatterHeads(torch.autograd.Function):
    """(H, Sl + T, D) local tensors (replicated text rows last) -> receive buffers of the rank's heads"""

    @staticmethod
    def forward(ctx, lay, order, *xs):
        Sl, T = lay.Sl, lay.T
        xs = [x.detach() for x in xs]
        bufs = [new_recv_buffer(lay) for _ in xs]
        lay.scatter_heads([x[:, :Sl] for x in xs], bufs, order, [x[:, Sl:] for x in xs] if T else None)
        ctx.lay, ctx.order = lay, list(order)
        return tuple(bufs)

    @staticmethod
    def backward(ctx, *gs):
        lay, order = ctx.lay, ctx.order
        Sl, T, me = lay.Sl, lay.T, lay.rank
        gs = [g.contiguous() for g in gs]
        dxs = [torch.empty((lay.H, Sl + T, lay.D), dtype=g.dtype, device=g.device) for g in gs]
        lay.gather_heads_multi(gs, [dx[:, :Sl] for dx in dxs], order)  # the tensors of one call travel together
        if T:
            mine = torch.as_tensor(order[lay.starts[me]:lay.starts[me + 1]], device=gs[0].device)
            for g, dx in zip(gs, dxs):
                dx[:, Sl:].zero_()
                dx[:, Sl:].index_copy_(0, mine, _text_view(lay, g))
        return (None, None, *dxs)


class _GatherHeads(torch.autograd.Function):
    """receive buffer of the rank's heads -> (Sl + T, H, D): the sequence shard of every head, then the gathered text rows"""

    @staticmethod
    def forward(ctx, lay, order, buf):
        Sl, T = lay.Sl, lay.T
        out = torch.empty((Sl + T, lay.H, lay.D), dtype=buf.dtype, device=buf.device)
        lay.gather_heads(buf.detach(), out[:Sl].transpose(0, 1), order, out[Sl:].transpose(0, 1) if T else None)
        ctx.lay, ctx.order = lay, list(order)
        return out

    @staticmethod
    def backward(ctx, g):
        lay, order = ctx.lay, ctx.order
        Sl, T = lay.Sl, lay.T
        g = g.contiguous()
        d_buf = new_recv_buffer(lay, g.dtype)
        # head shards <- sequence shards; the text rows: this rank's own heads of the (replicated) gradient
        lay.scatter_heads([g[:Sl].transpose(0, 1)], [d_buf], order, [g[Sl:].transpose(0, 1)] if T else None)
        return None, None, d_buf


def scatter_heads_autograd(lay: UlyssesLayout, xs: Sequence[torch.Tensor], head_order: Sequence[int]) -> List[torch.Tensor]:
    """`UlyssesLayout.scatter_heads` as a differentiable operator.  xs: (H, Sl + T, D) local tensors -- the sequence shard of
    every head with the replicated text rows at the end (any strides with contiguous channels).  Returns one fresh
    (rows_total, D) receive buffer per tensor (read it through `lay.head_view` and `lay.row_map`).  The backward sends the
    buffers' gradients back in one exchange, all tensors together; text rows get the gradient of the rank's own heads."""
    for x in xs:
        if x.dim() != 3 or tuple(x.shape) != (lay.H, lay.Sl + lay.T, lay.D):
            raise ValueError(f"scatter_heads_autograd takes ({lay.H}, {lay.Sl + lay.T}, {lay.D}) tensors, got {tuple(x.shape)}")
    return list(_ScatterHeads.apply(lay, list(head_order), *xs))


def gather_heads_autograd(lay: UlyssesLayout, buf: torch.Tensor, head_order: Sequence[int], token_major: bool = False):
    """`UlyssesLayout.gather_heads` as a differentiable operator: (sequence shard (H, Sl, D), text rows of all heads
    (H, T, D)), both views of one (Sl + T, H, D) tensor -- the layout the output projection reads; `token_major`: that
    tensor itself."""
    out = _GatherHeads.apply(lay, list(head_order), buf)
    return out if token_major else (out[:lay.Sl].transpose(0, 1), out[lay.Sl:].transpose(0, 1))
