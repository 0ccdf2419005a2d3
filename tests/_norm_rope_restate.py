"""Plain torch restatement of q/k RMSNorm + rotary embedding (include/vorta_hip.h vorta_qk_norm_rope), written from the
formulae and never from the kernels: the truth of the backward tests when run in float64, their yardstick when run in the
kernels' 16-bit dtype (torch's own autograd, one rounding per operator)."""
import torch


def norm_rope(x, w, eps, cos=None, sin=None, rope_tokens=0, across_heads=False):
    """x (H,S,D); w [D] or [H*D] (across_heads) or None; cos / sin (>= rope_tokens, D) or None.  Everything runs in x.dtype.
    y = x r w with r = rsqrt(mean(x^2) + eps), the mean over D or over all H*D channels of a token; rows < rope_tokens:
    out[2i] = y[2i] cos[2i] - y[2i+1] sin[2i],  out[2i+1] = y[2i+1] cos[2i+1] + y[2i] sin[2i+1]."""
    H, S, D = x.shape
    ms = x.pow(2).mean(dim=(0, 2), keepdim=True) if across_heads else x.pow(2).mean(dim=-1, keepdim=True)
    y = x * torch.rsqrt(ms + eps)
    if w is not None:
        y = y * (w.view(H, 1, D) if across_heads else w.view(1, 1, D))
    if cos is None or rope_tokens == 0:
        return y
    c, s = cos[:rope_tokens].to(x.dtype), sin[:rope_tokens].to(x.dtype)
    head = y[:, :rope_tokens]
    ye, yo = head[..., 0::2], head[..., 1::2]
    oe = ye * c[:, 0::2] - yo * s[:, 0::2]
    oo = yo * c[:, 1::2] + ye * s[:, 1::2]
    return torch.cat([torch.stack([oe, oo], dim=-1).flatten(-2), y[:, rope_tokens:]], dim=1)


def grads(x, g, w, eps, cos, sin, rope_tokens, across_heads, dtype):
    """(dx, dw | None) of sum(norm_rope(x) * g) by torch autograd with every tensor in `dtype`"""
    xl = x.detach().to(dtype).requires_grad_(True)
    wl = None if w is None else w.detach().to(dtype).requires_grad_(True)
    out = norm_rope(xl, wl, eps, cos, sin, rope_tokens, across_heads)
    got = torch.autograd.grad(out, [xl] if wl is None else [xl, wl], g.to(dtype))
    return got[0], (None if wl is None else got[1])


def rel_err(got, ref):
    got, ref = got.detach(), ref.detach()
    n = float(torch.linalg.norm(ref.double().reshape(-1)))
    return float(torch.linalg.norm(got.double().reshape(-1) - ref.double().reshape(-1))) / max(n, 1e-300)
