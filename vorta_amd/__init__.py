"""vorta_amd: VORTA's routed sparse-attention denoising path on MI355X (gfx950) -- hand-written HIP kernels behind the
reference's `vorta.attention` / `vorta.patch` / `vorta.ulysses` surface (the `vorta` package is an import alias)."""


def set_attention_precision(precision: str, *, measurement_only: bool = False) -> None:
    """"native" (contractions in the dtype of q,k,v, as the reference), "auto8" / "i8pv" / "fp8pv" (8-bit contractions on the
    int8 / fp8 MFMA with 16-bit output: BASELINE.json configs[4]; every one holds 40 dB against native on every input family
    tested).  Also: VORTA_ATTENTION_PRECISION in the environment.  "fp8" (e4m3 scores too) is measurement-only
    (vorta_amd/routed.py)."""
    from .routed import set_attention_precision as _set
    _set(precision, measurement_only=measurement_only)


def set_attention_backward(name: str) -> None:
    """"query_major" (the default: vorta_attn_bwd, dq bit-reproducible), "key_major" (a softmax-statistics pass, then a
    kernel that keeps dK / dV on chip and sums only dQ across workgroups) or "deterministic" (the statistics pass, a dQ pass
    and a dK / dV pass with one writer per row and no atomics: dq, dk and dv bit-reproducible) for the differentiable
    operators and processors, on one GPU and under sequence parallelism (there per rank: a sum across ranks is the training
    loop's).  Also: VORTA_ATTENTION_BACKWARD in the environment (vorta_amd/routed.py).  This switch is the only selector;
    torch.use_deterministic_algorithms does not change it."""
    from .routed import set_attention_backward as _set
    _set(name)


def set_partial_geometry(on: bool) -> None:
    """Accept tile and coreset windows that do not divide the latent grid (off by default; also VORTA_PARTIAL_GEOMETRY=0|1):
    thin last tiles for the sliding-tile expert, the reference's cropped windows plus full-resolution remainder tokens for the
    coreset expert (DESIGN.md "Partial geometry").  With it on, the published (6,9,8)/(2,3,2) geometry runs at 129 frames.
    A geometry that divides gives the same tables, launches and bits either way."""
    from ._partial import set_partial_geometry as _set
    _set(on)
