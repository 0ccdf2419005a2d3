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


def set_sliding_keys(name: str, mass_share=None) -> None:
    """Which key tiles the sliding-tile expert attends: "window" (the default: the clamped window of tiles around the query
    tile, the reference's mask), "content" (as many tiles, chosen per head and query tile on the device by the product of
    the tiles' mean q and mean k) or "mass" (as many tiles, chosen by the share of softmax mass that 16
    sampled query rows of the tile put on each key tile, scored on the matrix pipe).  Also:
    VORTA_SLIDING_KEYS=window|content|mass|share; read when a geometry is built.
    "share" keeps the FEWEST tiles, in the ranking of "mass", that hold the share `mass_share` (in (0, 1]) of the tile's sampled
    mass, at most the window's count, and runs the sliding expert as a launch whose key lists differ in length.
    It has no default share: give `mass_share=` here, to the geometry, or VORTA_SLIDING_MASS_SHARE.  Inference only, 16 bits.
    "content", "mass" and "share" are refused by name on a partial geometry, under sequence parallelism and in the per-expert sampled measurement
    (`sampled_expert_fidelity`, `route_by_fidelity`, `measured_routes`); "share" also in grad mode."""
    from .routed import set_sliding_keys as _set
    _set(name, mass_share)


def set_full_keys(name: str, mass_share=None) -> None:
    """Which keys the full-attention expert attends: "all" (the default: dense attention, the reference's expert) or "share": per
    head and query tile the FEWEST key tiles, in the ranking of sliding_keys="mass" but out of ALL tiles, that hold the share
    `mass_share` (in (0, 1]) of the tile's sampled attention mass, the tile itself first, then the text keys; text queries stay
    dense.  The heads run as one launch that walks tile lists of different lengths.  Also:
    VORTA_FULL_KEYS=all|share; read when a geometry is built.  No default share: give `mass_share=` here, `full_mass_share=` to the
    geometry, or VORTA_FULL_MASS_SHARE.  Inference only, 16 bits: refused by name on a partial geometry, under sequence
    parallelism, in grad mode and the soft-mixture operators, in the per-expert sampled measurement and under every 8-bit
    precision."""
    from .routed import set_full_keys as _set
    _set(name, mass_share)


def set_partial_geometry(on: bool) -> None:
    """Accept tile and coreset windows that do not divide the latent grid (off by default; also VORTA_PARTIAL_GEOMETRY=0|1):
    thin last tiles for the sliding-tile expert, the reference's cropped windows plus full-resolution remainder tokens for the
    coreset expert (DESIGN.md "Partial geometry").  With it on, the published (6,9,8)/(2,3,2) geometry runs at 129 frames.
    A geometry that divides gives the same tables, launches and bits either way."""
    from ._partial import set_partial_geometry as _set
    _set(on)
