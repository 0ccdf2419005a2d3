"""Routed sparse attention: the per-layer operator behind the attention processors.

Takes post-RoPE q,k,v (B,H,S[+T],D) and a head->expert assignment and enqueues, on the current stream,
at most:  1 launch for the full-attention heads, 2 selects + 1 launch for the coreset heads, and 1 (+1 for
Hunyuan's text queries) launch for the sliding-tile heads -- on a partial geometry (a tile that does not divide the
latent grid) one per key-list length, up to eight.  Every launch reads the original q,k,v through
head lists and row tables and writes its heads directly into the final output: the reference's per-expert
head gathers (hunyuan.py:612-640), pooled copies (coreset_select.py:68-124), tile/untile permutes
(tile.py) and boolean index-put (hunyuan.py:642-661) have no counterpart here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _partial, ops
from ._partial import partial_geometry, set_partial_geometry  # noqa: F401  (the switch: re-exported)

Triple = Tuple[int, int, int]


def _fold(x: torch.Tensor) -> torch.Tensor:
    """the (H,N,D) view the kernels take of a (1,H,N,D) or (H,N,D) tensor"""
    return x[0] if x.dim() == 4 else x


@dataclass
class HeadRouting:
    """head -> expert assignment.  Either host lists (counts known on the host) or the device tables written
    by ops.router_route (no host sync; every expert launch is sized for H slots and trims itself)."""
    lists: torch.Tensor                 # (3, H) int32 device, ascending heads per expert
    counts_host: Optional[List[int]]    # [n0,n1,n2] or None when only the device knows
    counts_dev: Optional[torch.Tensor]  # (3,) int32 device
    # full-attention heads that compute only a RANGE of their queries here (sequence parallelism below whole heads,
    # ulysses/engine.py split_placement): (one-entry int32 device list with the head, first query token, end); such a
    # head is not in lists[0]
    partials: Optional[List[Tuple[torch.Tensor, int, int]]] = None
    # the int32 (H,) head -> expert table on the device the lists were built from, where the maker has one: what
    # `routed_attention_repaired` rewrites in place beside the lists (None: the launches never read it)
    expert_ids: Optional[torch.Tensor] = None

    @staticmethod
    def from_expert_ids(expert_of_head: Sequence[int], device, q_ranges: Optional[dict] = None) -> "HeadRouting":
        """`q_ranges`: {head: (t0, t1)} for full-attention heads (expert 0) that attend only for query tokens [t0, t1)"""
        H = len(expert_of_head)
        q_ranges = q_ranges or {}
        lists = torch.zeros((3, H), dtype=torch.int32)
        counts = []
        for e in range(3):
            hs = [h for h, x in enumerate(expert_of_head) if int(x) == e and not (e == 0 and h in q_ranges)]
            counts.append(len(hs))
            if hs:
                lists[e, : len(hs)] = torch.tensor(hs, dtype=torch.int32)
        partials = None
        if q_ranges:
            if any(int(expert_of_head[h]) != 0 for h in q_ranges):
                raise ValueError("only full-attention heads (expert 0) can be split by query range")
            partials = [(torch.tensor([h], dtype=torch.int32).to(device), int(t0), int(t1))
                        for h, (t0, t1) in sorted(q_ranges.items())]
        return HeadRouting(lists.to(device), counts, None, partials)

    @staticmethod
    def from_device(lists: torch.Tensor, counts: torch.Tensor, expert_ids: Optional[torch.Tensor] = None) -> "HeadRouting":
        return HeadRouting(lists, None, counts, None, expert_ids)

    @staticmethod
    def every_head_everywhere(H: int, device) -> "HeadRouting":
        """all H heads on each of the three experts (the training-time soft mixture, hunyuan.py:375-396)"""
        lists = torch.arange(H, dtype=torch.int32).repeat(3, 1)
        return HeadRouting(lists.to(device), [H, H, H], None)

    def slot_args(self, e: int, H: int):
        if self.counts_host is not None:
            return dict(head_list=self.lists[e], n_heads=self.counts_host[e], n_heads_dev=None)
        return dict(head_list=self.lists[e], n_heads=H, n_heads_dev=self.counts_dev[e:e + 1])


class SampleTables(NamedTuple):
    """`RoutedGeometry.sample_tables`: the device tables of one (geometry, text length, sample table)"""
    tokens: torch.Tensor   # the sample table itself (kept alive: the cache is keyed on its address)
    order: torch.Tensor    # int64 (n,): compact row p holds sample position order[p]
    rows: torch.Tensor     # int32 (n,): the physical row of compact row p
    win: torch.Tensor      # int32 (n,): its coreset window, -1 outside the whole windows
    classes: list          # per sliding key-list length class: (start, count, kv_lists, stride, n_kv, block_table, n_lists)


def sample_launch_plan(latent, tile, window, group, tokens, t_eff: int = 0, block_rows: int = 256) -> dict:
    """Host integers of a per-expert measurement on the sampled video `tokens` (ascending ids in [0, S), raster order of the
    latent grid).  The sliding tile gives every query tile one key list (`_partial.window_geometry`: the first tile of its
    clamped window per dimension); lists of one LENGTH are one launch, longest first, as `sta_partial_launches` forms them
    (one class where the tile divides the grid: `sta_launch_tables`), and inside a launch the lists are in ascending order
    of (first tile) -- the rows of those tables.  Returns
      order   int64 (n,): the sample positions sorted by (class, list, position) -- compact row p holds tokens[order[p]]
      win     int32 (n,): in that order, the coreset window ((t // g0) ng1 + h // g1) ng2 + w // g2 of a token inside the ng =
              latent // group whole windows, else -1
      classes [dict(index, n_kv, n_lists, start, count, table)]: per length class that holds a sampled position, its index among
              ALL classes, its key count (video + t_eff), the number of its lists, its range [start, start + count) of compact
              rows and an int32 (blocks, 3) table of (list, first row, end row) -- rows relative to `start`, at most
              `block_rows` a block, no block across two lists."""
    import numpy as np
    tok = np.asarray(tokens, dtype=np.int64)
    L = [int(x) for x in latent]
    t, h, w = tok // (L[1] * L[2]), (tok // L[2]) % L[1], tok % L[2]
    nt, cnt, first = _partial.window_geometry(latent, tile, window)
    nf = [n - c + 1 for n, c in zip(nt, cnt)]
    fa = [np.asarray(first[d], dtype=np.int64) for d in range(3)]
    lid_of = lambda a, b, c: (fa[0][a] * nf[1] + fa[1][b]) * nf[2] + fa[2][c]  # noqa: E731
    grid = np.meshgrid(*(np.arange(n) for n in nt), indexing="ij")
    every = np.unique(lid_of(*grid))  # the lists some tile uses, ascending
    ext = [[_partial.list_extent(latent, tile, d, f, cnt[d]) for f in range(nf[d])] for d in range(3)]
    length = {int(l): ext[0][l // (nf[1] * nf[2])] * ext[1][(l // nf[2]) % nf[1]] * ext[2][l % nf[2]] + int(t_eff) for l in every}
    lengths = sorted(set(length.values()), reverse=True)
    members = [[l for l in every.tolist() if length[l] == n_kv] for n_kv in lengths]
    cls_of = {l: (ci, m.index(l)) for ci, m in enumerate(members) for l in m}
    lid = lid_of(t // int(tile[0]), h // int(tile[1]), w // int(tile[2]))
    ci = np.array([cls_of[int(l)][0] for l in lid], dtype=np.int64)
    gi = np.array([cls_of[int(l)][1] for l in lid], dtype=np.int64)
    order = np.lexsort((np.arange(tok.size), gi, ci)).astype(np.int64)
    ng = [l // int(g) for l, g in zip(L, group)]
    inside = (t < ng[0] * group[0]) & (h < ng[1] * group[1]) & (w < ng[2] * group[2])
    win = np.where(inside, ((t // group[0]) * ng[1] + h // group[1]) * ng[2] + w // group[2], -1).astype(np.int32)
    classes, start = [], 0
    for c, n_kv in enumerate(lengths):
        g_c = gi[order][ci[order] == c]
        if g_c.size == 0:
            continue
        table, p = [], 0
        for g in np.unique(g_c).tolist():
            end = p + int((g_c == g).sum())
            table += [(g, x, min(x + block_rows, end)) for x in range(p, end, block_rows)]
            p = end
        classes.append(dict(index=c, n_kv=n_kv, n_lists=len(members[c]), start=start, count=int(g_c.size),
                            table=np.asarray(table, dtype=np.int32)))
        start += int(g_c.size)
    return dict(order=order, win=win[order], classes=classes)


@dataclass
class RoutedGeometry:
    """Everything that depends only on (latent, tile, window, coreset window, rate, text length).
    Built once per run / prompt, like the reference's LowresGroupInfo + BlockMask
    (vorta/patch/utils.py:8-56, pipeline_hunyuan.py:378-392)."""
    latent: Triple
    tile: Triple
    window: Triple
    group: Triple
    rate: float
    device: torch.device
    row_map: Optional[torch.Tensor] = None  # zero-copy Ulysses layout (ulysses.py); None = plain (H,S,D)
    _sta: Dict[int, Tuple[torch.Tensor, torch.Tensor, int]] = field(default_factory=dict)
    # accept a tile / coreset window that does not divide the latent grid (DESIGN.md "Partial geometry"); None = the
    # process-wide switch (set_partial_geometry / VORTA_PARTIAL_GEOMETRY).  A geometry that divides is built as ever.
    partial: Optional[bool] = None

    def __post_init__(self):
        self.latent, self.tile, self.window, self.group = (tuple(int(v) for v in x) for x in
                                                           (self.latent, self.tile, self.window, self.group))
        self.S = self.latent[0] * self.latent[1] * self.latent[2]
        self.g = self.group[0] * self.group[1] * self.group[2]
        self.partial = partial_geometry() if self.partial is None else bool(self.partial)
        # is_partial: the tables, launches and lists below differ from the dividing ones only then
        self.is_partial = self.partial and not _partial.divides(self.latent, self.tile, self.group)
        self.n_keep = int(self.g * (1 - self.rate)) - 1  # coreset_select.py:54
        # the distinct VIDEO key counts of the sliding expert's key lists, longest first (one where the tile divides)
        self.sta_class_n_kv = _partial.sliding_key_counts(self.latent, self.tile, self.window)
        if self.is_partial:
            # G: the whole windows the reference keeps when it crops (coreset_select.py:36-40); C: the tokens outside the
            # cropped box -- full resolution, never duplicated
            self.G, _, self.C, self.S_low = _partial.coreset_numbers(self.latent, self.group, self.rate)
            self.tok = None  # tiles differ in size
            return
        self.C = 0
        for l, t in zip(self.latent, self.tile):
            if l % t:
                # same condition and exception type as hunyuan.py:264-267
                raise ValueError(f"Tile size {self.tile} (dim={t}) does not divide latent shape {self.latent} (dim={l}).")
        self.G = 1
        for l, w in zip(self.latent, self.group):
            self.G *= l // w
        if self.S != self.G * self.g:
            raise ValueError(f"Input sequence length {self.S} does not match low-res info {self.G}x{self.g}.")
        self.S_low = self.G * (1 + self.n_keep)
        self.tok = self.tile[0] * self.tile[1] * self.tile[2]

    def sta_partial_launches(self, t_eff: int, block_rows: int = 256):
        """The sliding-tile expert on a partial geometry: one merged launch per key-list LENGTH (the attention kernel takes
        one n_kv per launch).  Query tiles of equal key lists form a group, as in `sta_launch_tables`; the groups of one
        length class are one launch with its own q_rows, key lists and block table, longest class first.  Together the
        classes hold every query position once (tiles partition the grid, a tile has one key list, a list one length).
        Returns a list of (q_rows (n_q,), kv_lists (n_lists, stride), stride, n_kv, block_table, n_lists)."""
        key = ("partial", t_eff, block_rows)
        if key not in self._sta:
            q_rows, kv_rows, lens = ops.sta_build_tables_partial(self.latent, self.tile, self.window, t_eff, self.device,
                                                                 row_map=self.row_map)
            stride = kv_rows.shape[1]
            nt, cnt, first = _partial.window_geometry(self.latent, self.tile, self.window)
            nf = [n - c + 1 for n, c in zip(nt, cnt)]
            thick = [[min(self.tile[d], self.latent[d] - i * self.tile[d]) for i in range(nt[d])] for d in range(3)]
            by_list: Dict[int, list] = {}  # key list -> [(first position, tokens)] of its tiles, tile-major
            start = 0
            for a in range(nt[0]):
                for b in range(nt[1]):
                    for c in range(nt[2]):
                        n = thick[0][a] * thick[1][b] * thick[2][c]
                        lid = (first[0][a] * nf[1] + first[1][b]) * nf[2] + first[2][c]
                        by_list.setdefault(lid, []).append((start, n))
                        start += n
            assert start == self.S
            launches = []
            for n_kv in sorted({lens[l] for l in by_list}, reverse=True):
                lids = sorted(l for l in by_list if lens[l] == n_kv)
                pos, rows, p0 = [], [], 0
                for g, l in enumerate(lids):
                    end = p0 + sum(n for _, n in by_list[l])
                    pos += [torch.arange(s, s + n) for s, n in by_list[l]]
                    rows += [(g, p, min(p + block_rows, end)) for p in range(p0, end, block_rows)]
                    p0 = end
                q_c = q_rows[torch.cat(pos).to(self.device)].contiguous()
                lists = kv_rows[torch.tensor(lids, device=self.device)].contiguous()
                table = torch.tensor(rows, dtype=torch.int32).to(self.device)
                launches.append((q_c, lists, stride, n_kv, table, len(lids)))
            assert sum(x[0].numel() for x in launches) == self.S
            self._sta[key] = launches
        return self._sta[key]

    def sta_tables(self, t_eff: int):
        """per query tile: (q_rows (S,), kv_rows (n_tiles, n_kv), n_kv) -- vorta_sta_build_tables"""
        if self.is_partial:
            raise ValueError("a partial geometry has no per-tile table of one length: sta_partial_launches")
        if t_eff not in self._sta:
            q_rows, kv_rows = ops.sta_build_tables(self.latent, self.tile, self.window, t_eff, self.device,
                                                   row_map=self.row_map)
            self._sta[t_eff] = (q_rows, kv_rows, kv_rows.shape[1])
        return self._sta[t_eff]

    def prebuild(self, t_eff: int, block_rows: int = 256) -> None:
        """Build (on the CURRENT stream) every lazily cached device table a routed call with this text length may touch.
        Callers that enqueue routed_attention on several streams call this before they fork: a table built inside one
        stream's call is not ordered against another stream's first use of the cached object."""
        if self.is_partial:
            self.sta_partial_launches(t_eff, block_rows if block_rows in (128, 256) else 256)
            return
        self.sta_tables(t_eff)
        if STA_MERGE and block_rows in (128, 256):
            self.sta_launch_tables(t_eff, block_rows)

    def sample_tables(self, t_eff: int, tokens: torch.Tensor, block_rows: int = 256) -> "SampleTables":
        """What `sampled_expert_fidelity` needs beside the sample itself, built ONCE per (text length, sample table) -- host
        work (`sample_launch_plan`, which reads `tokens` back) -- and cached beside the `_sta` tables: the position order,
        the physical rows and coreset windows in that order, and per key-list length class of the sliding expert the
        positions' range, the key lists of `sta_launch_tables` / `sta_partial_launches` and a block table of its own.  The
        cache holds `tokens`, so its address is not handed to another table."""
        key = ("sample", t_eff, block_rows, tokens.data_ptr(), tokens.numel(), tokens._version)
        if key not in self._sta:
            plan = sample_launch_plan(self.latent, self.tile, self.window, self.group, tokens.cpu().numpy(), t_eff, block_rows)
            if self.is_partial:
                full = [(x[1], x[2], x[3], x[5]) for x in self.sta_partial_launches(t_eff, block_rows)]
            else:
                _, lists, n_kv, _, n_lists = self.sta_launch_tables(t_eff, block_rows)
                full = [(lists, n_kv, n_kv, n_lists)]
            classes = []
            for c in plan["classes"]:
                lists, stride, n_kv, n_lists = full[c["index"]]
                assert (n_kv, n_lists) == (c["n_kv"], c["n_lists"]), "the host plan and the device tables disagree on a class"
                classes.append((c["start"], c["count"], lists, stride, n_kv, torch.from_numpy(c["table"]).to(self.device), n_lists))
            order = torch.from_numpy(plan["order"]).to(self.device)
            toks = tokens.index_select(0, order)
            rows = toks if self.row_map is None else self.row_map.index_select(0, toks)
            self._sta[key] = SampleTables(tokens, order, rows.contiguous(), torch.from_numpy(plan["win"]).to(self.device), classes)
        return self._sta[key]

    def sta_launch_tables(self, t_eff: int, block_rows: int = 256):
        """The sliding-tile launch with query tiles of EQUAL key lists merged into one group.  The reference clamps the
        window centre (sliding_attn_flex.py:118-120), so the two outermost tiles of a dimension -- all tiles, when the
        dimension has no more tiles than the window -- see the same keys: Hunyuan-129f has 150 query tiles and 24
        distinct key lists.  Merged, a group is 3, 6 or 12 tiles long and is cut into full 256-row workgroups (2-7 %
        padding) where every single 792-token tile ended in a 24-row one (29 %).
        Returns (q_rows (S,), kv_lists (n_lists, n_kv), n_kv, block_table (n_blocks, 3) int32, n_lists)."""
        key = ("merged", t_eff, block_rows)
        if key not in self._sta:
            q_rows, kv_rows, n_kv = self.sta_tables(t_eff)
            n_tiles = kv_rows.shape[0]
            # a tile's key list is fixed by the first tile of its clamped window in every dimension: host integers
            nt, _, first = _partial.window_geometry(self.latent, self.tile, self.window)
            ids = [(first[0][a], first[1][b], first[2][c]) for a in range(nt[0]) for b in range(nt[1]) for c in range(nt[2])]
            order = sorted(range(n_tiles), key=lambda i: ids[i])  # stable: tile-major order kept inside a group
            groups = []  # (first tile of the group, number of tiles)
            for i in order:
                if groups and ids[groups[-1][0]] == ids[i]:
                    groups[-1][1] += 1
                else:
                    groups.append([i, 1])
            order_t = torch.tensor(order, device=self.device)
            q_m = q_rows.view(n_tiles, self.tok)[order_t].reshape(-1).contiguous()
            lists = kv_rows[torch.tensor([g[0] for g in groups], device=self.device)].contiguous()
            rows, start = [], 0
            for g, (_, c) in enumerate(groups):
                end = start + c * self.tok
                rows += [(g, p, min(p + block_rows, end)) for p in range(start, end, block_rows)]
                start = end
            table = torch.tensor(rows, dtype=torch.int32).to(self.device)
            self._sta[key] = (q_m, lists, n_kv, table, len(groups))
        return self._sta[key]


def _auto_splits(n_heads: int, n_q: int, n_kv: int) -> int:
    """Few query rows against a long key list: cut the keys so the launch fills the chip (256 CUs)."""
    qblocks = max(1, (n_q + 255) // 256) * max(1, n_heads)
    kv_blocks = (n_kv + 63) // 64
    want = max(1, 512 // qblocks)
    return max(1, min(want, kv_blocks // 8 if kv_blocks >= 16 else 1, 256))


from ._debug import flag as _debug_flag  # the A/B switches below sit behind ONE gate: VORTA_DEBUG="key=value,..." (_debug.py)
# merge query tiles of equal key lists into one group of the sliding-tile launch (RoutedGeometry.sta_launch_tables);
# sta_merge=0: one group per tile, as round 1 (A/B)
STA_MERGE = _debug_flag("sta_merge", "1") != "0"
# process-wide default of `routed_attention(fp8=None)`: the processors of vorta.attention call it that way, so the
# unchanged inference scripts pick an 8-bit path up from the environment or from `set_attention_precision(...)`:
# False (native), "fp8pv" (16-bit scores, e4m3 P V), "i8pv" (int8 scores: one key scale per head, one query scale per wave;
# e4m3 P V) or "auto8" (per head one of the two).  True = both contractions in e4m3 is NOT a product precision (round 6,
# VERDICT r05): 20.8-35.7 dB on structured inputs against the 40 dB bar; measurements reach it through
# `routed_attention(fp8=True)`, `bench.py --dtype fp8` and `set_attention_precision("fp8", measurement_only=True)`.
PRODUCT_PRECISIONS = ("native", "fp8pv", "i8pv", "auto8")
_NOT_A_PRODUCT = ("'fp8' (q k^T AND P V in e4m3) is not a product precision: 3 mantissa bits on the scores give 20.8-35.7 dB on "
                  "structured inputs (40.1 dB only on white noise; DESIGN.md (c)) against the 40 dB bar.  Use 'auto8' (int8 or "
                  "16-bit scores per head, e4m3 P V: >= 40.9 dB on every input family, 1.6 x bf16), 'i8pv' or 'fp8pv'; the "
                  "all-e4m3 kernels stay reachable for measurements: bench.py --dtype fp8, routed_attention(fp8=True), "
                  "set_attention_precision('fp8', measurement_only=True)")
_PREC_ENV = __import__("os").environ.get("VORTA_ATTENTION_PRECISION", "").lower()
if _PREC_ENV == "fp8":
    raise ValueError("VORTA_ATTENTION_PRECISION=fp8: " + _NOT_A_PRODUCT)
if _PREC_ENV not in ("",) + PRODUCT_PRECISIONS:
    raise ValueError(f"VORTA_ATTENTION_PRECISION={_PREC_ENV!r}: one of {PRODUCT_PRECISIONS}")
DEFAULT_FP8 = _PREC_ENV if _PREC_ENV in ("fp8pv", "i8pv", "auto8") else False
# the e4m3 conversion subtracts a per-head centre from the keys (softmax-invariant, buys back what a common component of
# the keys costs in e4m3: include/vorta_hip.h vorta_fp8_quant_args.flags); fp8_center_k=0 turns it off (A/B)
FP8_CENTER_K = _debug_flag("fp8_center_k", "1") != "0"
# coreset expert, key side: coreset_kv_order=group reads K/V through a group-major ascending row list (the same rows
# as the reference's packed [centres | margins] list; softmax does not see key order).  Measured NEUTRAL at Hunyuan-129f
# fp16 (coreset launch 1 111 vs 1 109 TFLOP/s, fused step 4 099 vs 4 094 ms, profiles/r03_coreset_kv_order.txt): the
# launch's distance from the full-attention one is its tail (7.3 rounds of workgroups) and the row tables, not the
# gather's locality -- so the default stays the reference's order.
CORESET_KV_GROUP_MAJOR = _debug_flag("coreset_kv_order", "packed") == "group"
# fused grid: the sliding expert's text-query segment goes first with at most this many key splits (0: as round 1 -- last,
# with the stand-alone launch's split count; A/B)
FUSED_TEXT_SPLITS = int(_debug_flag("fused_text_splits", "1"))
FUSED_TEXT_FIRST = FUSED_TEXT_SPLITS > 0


def set_attention_precision(precision: str, *, measurement_only: bool = False) -> None:
    """"native" (the dtype of q,k,v: the reference's behaviour), "fp8pv" (scores in 16 bits, P V in e4m3: >= 41 dB on every
    input family tried), "i8pv" (scores in int8 at the e4m3 MFMA rate, P V in e4m3: >= 40 dB on every family, relative error
    <= 0.07 on all but heavy-tailed inputs) or "auto8" ("i8pv" per head, with 16-bit scores -- "fp8pv" -- for the heads whose
    int8 keys would be too coarse; chosen on the device); 16-bit output in every case.  Every product
    precision holds the 40 dB bar on all seven input families of tests/_fp8_inputs.py at full size.
    "fp8" (both contractions in e4m3) does not -- 20.8-35.7 dB on structured inputs -- and is refused unless
    `measurement_only=True` (bench.py, the kernel tests)."""
    global DEFAULT_FP8
    if precision == "fp8":
        if not measurement_only:
            raise ValueError(_NOT_A_PRODUCT)
        DEFAULT_FP8 = True
        return
    if precision not in PRODUCT_PRECISIONS:
        raise ValueError(f"precision is one of {PRODUCT_PRECISIONS}")
    DEFAULT_FP8 = precision if precision in ("fp8pv", "i8pv", "auto8") else False


PRECISIONS = ("native", "fp8", "fp8pv", "i8pv", "auto8")


def precision_of(fp8) -> str:
    """the precision name of an `fp8=` value: None = the process default (DEFAULT_FP8), False = "native", True = "fp8"
    (both contractions in e4m3), or a name of PRECISIONS"""
    fp8 = DEFAULT_FP8 if fp8 is None else fp8
    if isinstance(fp8, str) and fp8 not in PRECISIONS:
        raise ValueError(f"attention precision {fp8!r}: one of {PRECISIONS}")
    return fp8 if isinstance(fp8, str) else "fp8" if fp8 else "native"


class AttnOperands(NamedTuple):
    """What one precision hands the attention kernels: q, k, v as the launches read them, `v_descale` of an e4m3 v, `i8`
    the I8Operands of int8 keys; "auto8" adds the 16-bit keys `k16` and the heads' tail flags `tail` (ops.i8_tail_flags)."""
    precision: str
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    v_descale: Optional[torch.Tensor] = None
    i8: Optional["ops.I8Operands"] = None
    k16: Optional[torch.Tensor] = None
    tail: Optional[torch.Tensor] = None

    def kwargs(self, scale: Optional[float]) -> dict:  # of ops.attn_fwd ("auto8": its int8-score launch)
        return dict(q=self.q, k=self.k, v=self.v, scale=scale, v_descale=self.v_descale, i8=self.i8)

    def tail_kwargs(self, scale: Optional[float]) -> dict:  # "auto8": the 16-bit-score launch of the flagged heads
        return dict(q=self.q, k=self.k16, v=self.v, scale=scale, v_descale=self.v_descale)


def prepare_operands(precision: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float],
                     fp8_operands=None, video_tokens: int = 0) -> AttnOperands:
    """the operands of a one-GPU call: (H,S,D) q, k, v converted for `precision`.  `fp8_operands`: buffers to reuse -- an
    ops.Fp8Operands ("fp8"), the tuple of ops.fp8_quantize_v ("fp8pv") or (that tuple, ops.I8Operands) ("i8pv", "auto8")"""
    reuse = isinstance(fp8_operands, tuple)
    if precision in ("i8pv", "auto8"):
        # int8 scores: k -> int8 rows (centred, balanced, one scale per head) + a float bias per row, v -> e4m3; q is centred,
        # balanced and rounded by the attention kernel itself.  "auto8": per head, int8 scores where the head's int8 keys
        # resolve their bulk, 16-bit scores where they do not (heavy tails).  The choice is made on the device (the tail
        # flags here, ops.split_heads over every expert's head list): two fused launches per layer, one of them usually over
        # empty lists (its workgroups exit in their first instruction), no host synchronisation
        vo, ko = fp8_operands if reuse and len(fp8_operands) == 2 else (None, None)
        v8, vd, _ = ops.fp8_quantize_v(v, out=vo)
        i8 = ops.i8_quantize_k(q, k, out=ko)
        tail = ops.i8_tail_flags(i8.k8) if precision == "auto8" else None
        return AttnOperands(precision, q, i8.k8, v8, vd, i8, None if tail is None else k, tail)
    if precision == "fp8pv":  # scores in 16 bits, P V in e4m3: only v is converted (exact per-channel abs-max, one pass + one)
        v8, vd, _ = ops.fp8_quantize_v(v, out=fp8_operands if reuse and len(fp8_operands) == 3 else None)
        return AttnOperands(precision, q, k, v8, vd)
    if precision == "fp8":
        f8 = ops.fp8_quantize_qkv(q, k, v, scale, out=fp8_operands, center_k=FP8_CENTER_K, video_tokens=video_tokens)
        return AttnOperands(precision, f8.q, f8.k, f8.v, f8.v_descale)
    return AttnOperands("native", q, k, v)


_SIDE_STREAMS: Dict[int, Tuple[torch.cuda.Stream, torch.cuda.Stream]] = {}

# ---- routed-output fidelity on sampled dense query rows ---------------------------------------------------
DEFAULT_FIDELITY_ROWS = 2048  # sampled video rows per head: 1.7 % of Hunyuan-129f's 118 800 (by FLOP count, of a dense head)
FIDELITY_HEADS = ("sparse", "all")
# key splits of the dense reference launches: n query rows against every key are a few workgroups per head, each with the
# longest key loop there is, so the keys are cut into this many parts (+ a merge kernel) where every part keeps 8 key blocks
# (`fidelity_ref_splits`).  The cut follows from the KEY COUNT alone -- not from n, the head count or the form of the head
# lists -- so the reference rows, whose summation order the cut decides, have the same bits for host and device lists, every
# sample size and every rank.  1 leaves the keys whole (the A/B of tools/bench_routed_fidelity.py, which sets this in its own
# process: profiles/routed_fidelity_timing.json)
FIDELITY_REF_SPLITS = 8
_SAMPLE_ROWS: Dict[tuple, torch.Tensor] = {}  # (S, n, seed, device) -> table; a table handed out is never evicted (a graph may read it)


def fidelity_ref_splits(n_kv: int) -> int:
    """the key parts of a dense reference launch over `n_kv` keys: FIDELITY_REF_SPLITS, fewer where a part would fall under 8
    key blocks of 64 (one part under 16 blocks)"""
    return max(1, min(int(FIDELITY_REF_SPLITS), ((n_kv + 63) // 64) // 8))


def sample_rows(S: int, n: int, seed: int = 0, device=None) -> torch.Tensor:
    """The `n` video tokens of [0, S) on which the routed output is compared with dense attention: a stratified random table,
    int32 (n,), ascending and distinct by construction.  Stratum i is [floor(i S / n), floor((i + 1) S / n)); one token per
    stratum, lo + floor(u (hi - lo)) with u = numpy.random.default_rng(seed).random(n), drawn on the host.  Stratified, so
    that every part of the clip is seen; random inside a stratum, so that no stride locks onto the in-window position of the
    coreset windows or onto a tile phase.  n == S gives every row; n > S is a ValueError.  Built once per (S, n, seed) and
    cached, on `device` when one is given (None: the host table); a cached table is never freed, so a captured graph that
    reads one stays valid."""
    import numpy as np
    S, n, seed = int(S), int(n), int(seed)
    if n > S or n < 0:
        raise ValueError(f"a sample of {n} rows out of {S} video tokens")
    key = (S, n, seed, None if device is None else str(torch.device(device)))
    if key not in _SAMPLE_ROWS:  # (4 n bytes a table, kept for the life of the process: a captured graph reads its address)
        host = _SAMPLE_ROWS.get(key[:3] + (None,))
        if host is None:
            i = np.arange(n, dtype=np.int64)
            lo, hi = (i * S) // n if n else i, ((i + 1) * S) // n if n else i
            u = np.random.default_rng(seed).random(n)
            tok = np.minimum(lo + np.floor(u * (hi - lo)).astype(np.int64), hi - 1)  # (u < 1: the minimum never binds)
            host = _SAMPLE_ROWS[key[:3] + (None,)] = torch.from_numpy(tok.astype(np.int32))
        if device is not None:
            _SAMPLE_ROWS[key] = host.to(device)
    return _SAMPLE_ROWS[key]


def _named_heads(slot: torch.Tensor, count, head_list: torch.Tensor, H: int) -> torch.Tensor:
    """per slot of a head list the head it names, int64 on the device without a host read: H -- one past the heads -- for a
    slot at or past `count` (a host integer or a device count), which no launch reads"""
    heads = head_list[:slot.numel()].long()
    return torch.where(slot < count, heads, torch.full_like(heads, H))


def _expert_ids(routing: "HeadRouting", H: int, device) -> torch.Tensor:
    """head -> expert as the launches read it, int32 (H,) on the device without a host read: -1 for a head no list names;
    a head split by query range is a full-attention head (0)"""
    ids = torch.full((H + 1,), -1, dtype=torch.int32, device=device)
    slot = torch.arange(H, device=device)
    for e in range(3):
        count = routing.counts_host[e] if routing.counts_host is not None else routing.counts_dev[e]
        ids.scatter_(0, _named_heads(slot, count, routing.lists[e], H), torch.full((H,), e, dtype=torch.int32, device=device))
    for hl, _, _ in routing.partials or ():
        ids.index_fill_(0, hl.long(), 0)
    return ids[:H]


def _sample_table(rows, S: int, seed: int, device, name: str) -> torch.Tensor:
    """`rows` -- a sample size (None: min(DEFAULT_FIDELITY_ROWS, S); `sample_rows` with `seed`) or an int32 table of video
    tokens -- as the table; `name`: the caller's argument, for the message"""
    if rows is None:
        rows = min(DEFAULT_FIDELITY_ROWS, S)
    tokens = rows if torch.is_tensor(rows) else sample_rows(S, rows, seed, device)
    if tokens.dim() != 1 or tokens.dtype != torch.int32 or tokens.numel() > S:
        raise ValueError(f"{name}: a sample size, or an int32 table of video tokens (routed.sample_rows)")
    return tokens


def _measure_routed(fidelity: list, fidelity_rows, fidelity_heads: str, q3, k3, v3, o3, routing: "HeadRouting",
                    geom: "RoutedGeometry", te: int, scale: Optional[float]) -> None:
    """`routed_attention(fidelity=...)`: dense attention in the input dtype on the sampled query rows of the measured heads
    (the 16-bit q gathered at the rows, every valid key: ops.attn_fwd as expert 0 passes its key side), compared with the
    rows the routed launches wrote (ops.sampled_fidelity, `out` read in place); files one ops.SampledFidelity"""
    if fidelity_heads not in FIDELITY_HEADS:
        raise ValueError(f"fidelity_heads={fidelity_heads!r}: one of {FIDELITY_HEADS}")
    H, S, rm = q3.shape[0], geom.S, geom.row_map
    tokens = _sample_table(fidelity_rows, S, 0, q3.device, "fidelity_rows")
    n = tokens.numel()
    rows = tokens if rm is None else rm.index_select(0, tokens)  # the physical rows of q and out
    q_rows = q3.index_select(1, rows)       # compact (H, n, D): the launch below has no query table
    ref = torch.empty_like(q_rows)
    key_side = dict(n_kv=S + te, kv_rows=None if rm is None else rm[:S + te], scale=scale)
    splits = fidelity_ref_splits(S + te)
    stats = None
    for e in ((1, 2) if fidelity_heads == "sparse" else (0, 1, 2)):
        # (heads split by query range, routing.partials, are in no list: not measured)
        if routing.counts_host is not None and routing.counts_host[e] == 0:
            continue
        slots = routing.slot_args(e, H)
        if n:
            ops.attn_fwd(q_rows, k3, v3, ref, n_q=n, q_valid=n, n_splits=splits, tag="fidelity_ref", **key_side, **slots)
        stats = ops.sampled_fidelity(ref, o3, rows, **slots, into=stats)
    if stats is None:  # no head to measure: every statistic NaN
        stats = ops.sampled_fidelity(ref, o3, rows, n_heads=0)
    fidelity.append(stats._replace(rows=tokens, expert=_expert_ids(routing, H, q3.device)))


SAMPLED_BLOCK_ROWS = 256  # workgroup rows of the sampled coreset and sliding launches: the body the routed launches run


def _head_slots(heads, H: int, device) -> dict:
    """`heads=` of `sampled_expert_fidelity` -> head_list / n_heads / n_heads_dev as the launches read them"""
    if heads is None:
        return dict(head_list=None, n_heads=H, n_heads_dev=None)
    if isinstance(heads, dict):
        return dict(head_list=heads["head_list"], n_heads=heads["n_heads"], n_heads_dev=heads.get("n_heads_dev"))
    if isinstance(heads, tuple) and len(heads) == 2 and torch.is_tensor(heads[0]):
        return dict(head_list=heads[0], n_heads=heads[0].numel(), n_heads_dev=heads[1])
    if not torch.is_tensor(heads):
        heads = torch.tensor([int(h) for h in heads], dtype=torch.int32).to(device)
    return dict(head_list=heads, n_heads=heads.numel(), n_heads_dev=None)


def _coreset_lists(q3, k3, geom: "RoutedGeometry", hy: bool, T: int, te: int, slots: dict):
    """the coreset expert's selection for the heads of `slots`: (keep_q, drop_q, keep_k) of ops.coreset_select"""
    S, rm = geom.S, geom.row_map
    # key side: the same rows as the reference's packed [centres | margins] list (coreset_select.py:116-124) in
    # group-major ascending order -- softmax does not see the order of the keys, the K/V gather does
    gm = CORESET_KV_GROUP_MAJOR
    pk = dict(partial=True) if geom.is_partial else {}  # + the remainder tokens, before the text (vorta_coreset_select_partial)
    if hy:  # K matched on its own, V follows K (hunyuan.py:433-438)
        keep_q, drop_q = ops.coreset_select(q3, geom.latent, geom.group, geom.n_keep, tail_first=S, n_tail=T,
                                            row_map=rm, **pk, **slots)
        kk = ops.coreset_select(k3, geom.latent, geom.group, geom.n_keep, tail_first=S, n_tail=te, row_map=rm,
                                want_drop=False, want_keep=not gm, want_kv=gm, **pk, **slots)
        return keep_q, drop_q, kk[2] if gm else kk[0]
    # K and V follow Q's matching (wan.py:250-255): one selection, both lists
    kq = ops.coreset_select(q3, geom.latent, geom.group, geom.n_keep, tail_first=S, n_tail=T, row_map=rm,
                            want_kv=gm, **pk, **slots)
    return kq[0], kq[1], kq[2] if gm else kq[0]


def _full_launch(geom: "RoutedGeometry", T: int, te: int, kv_splits) -> dict:
    """the lengths and row tables of full attention over every head row -- expert 0, and the dense repair launch: every query
    (text included), every valid key; the keys cut where `kv_splits` > 1"""
    S, rm = geom.S, geom.row_map
    return dict(n_q=S + T, n_kv=S + te, q_valid=S + te, q_rows=None if rm is None else rm[:S + T],
                kv_rows=None if rm is None else rm[:S + te],
                **(dict(n_splits=int(kv_splits)) if kv_splits and int(kv_splits) > 1 else {}))


def sampled_expert_fidelity(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, geom: RoutedGeometry, *, model: str,
                            text_len: int = 0, text_valid: int = 0, scale: Optional[float] = None, rows=None, seed: int = 0,
                            out: Optional[torch.Tensor] = None, heads=None, outputs: Optional[list] = None,
                            precision: Optional[str] = None, operands: Optional[AttnOperands] = None
                            ) -> "ops.ExpertFidelity":
    """What EVERY expert would have written for a head, on a sample of video rows: an `ops.ExpertFidelity` (column 0 coreset,
    column 1 sliding tile against dense attention on the same rows) without the soft mixture's three full-size forwards.
    q, k, v: as `routed_attention` takes them, (1,H,S[+T],D) or (H,..); the contractions run in their dtype, whatever
    VORTA_ATTENTION_PRECISION says (this measures the method, not a precision).
    rows: a sample size (None: min(DEFAULT_FIDELITY_ROWS, S); `sample_rows` with `seed`) or an int32 table of `sample_rows`.
    Per call, all on the current stream and without a host read (graph-capturable once `geom.sample_tables` is built):
    `ops.coreset_select` for the measured heads as the coreset expert calls it; one `ops.gather_sample_rows`; dense attention
    on the rows' queries as `routed_attention(fidelity=...)` forms it (keys cut by `fidelity_ref_splits`); the coreset expert's
    value at a row = its REPRESENTATIVE query (the row, or its window's centre where the head's selection dropped it) against
    the head's keep list; the sliding tile's value = the row's query against its tile's key list, one launch per key-list
    length with the positions ordered by key list; then `ops.expert_fidelity` on the three compact buffers.  The coreset and
    sliding launches cut their keys by `fidelity_ref_splits(n_kv)` too -- by the key count alone, so records compare.  The
    launches go to `ops.attn_fwd_batch`, which fuses those that qualify; every launch writes rows of its own.
    out: the output of a routed call on the same q, k, v: column 2 of the record is then that output AS LAUNCHED against dense
    attention (NaN without); `out` is only read.
    heads: None = every head; else a sequence of head ids, an int32 device list, a (list, device count) pair or the
    head_list / n_heads / n_heads_dev dictionary of `HeadRouting.slot_args`.  Heads not measured hold NaN.
    outputs: a list that receives the compact (H, n, D) buffers -- dense, coreset, sliding (and the rows of `out`) -- and last
    the int64 position order: compact row p is sample position order[p] (rows are ordered by sliding key list).
    precision: None (above), or "fp8pv" / "i8pv" = the measurement IN THAT TIER'S PRECISION: the dense reference rows stay in
    the input dtype; the coreset and the sliding launches read that precision's operands (K, V converted once per call by
    `prepare_operands`, or `operands=` the AttnOperands the caller prepared for this precision -- "auto8" operands serve both
    tiers -- and goes on to launch with); and a third compact launch runs FULL attention on the rows' own queries in that
    precision, whose error is column 2 (the `mixed` slot of `ops.expert_fidelity`), and whose buffer `outputs` receives in the
    place of the rows of `out`.  `precision` together with `out=` is a ValueError (column 2 holds one of the two).  The
    coreset ranking still reads the 16-bit q, k, as the routed launches' does.  No host read; graph-capturable.  What the
    record of a tier bounds: these launches on these rows.  A full-size launch of the same tier is the same arithmetic with
    another key cut (`fidelity_ref_splits` against the routed call's own) and, under "i8pv", another grouping of rows into
    waves (the int8 query scale is a wave's, over its 32 rows: DESIGN.md 6.8)."""
    hy = model == "hunyuan"
    if precision is not None:
        if precision not in ("fp8pv", "i8pv"):
            raise ValueError(f"sampled_expert_fidelity: precision={precision!r} (None, 'fp8pv' or 'i8pv')")
        if out is not None:
            raise ValueError("sampled_expert_fidelity: precision= together with out=: column 2 holds full attention in that "
                             "precision or the routed output, not both")
    elif operands is not None:
        raise ValueError("sampled_expert_fidelity: operands= goes with precision=")
    q3, k3, v3 = _fold(q), _fold(k), _fold(v)
    o3 = None if out is None else _fold(out)
    H, D, S, rm = q3.shape[0], q3.shape[-1], geom.S, geom.row_map
    T, te = (text_len, text_valid) if hy else (0, 0)
    if rm is None and q3.shape[1] != S + T:
        raise ValueError(f"Input sequence length {q3.shape[1] - T} does not match latent shape {geom.latent}.")
    tokens = _sample_table(rows, S, seed, q3.device, "rows")
    n, dev = tokens.numel(), q3.device
    sl = _head_slots(heads, H, dev)
    tabs = geom.sample_tables(te, tokens, SAMPLED_BLOCK_ROWS)
    # every row of a buffer the statistics pass reads is written only for the measured heads: the others hold zeros
    new = torch.empty if sl["head_list"] is None else torch.zeros
    q_own, q_rep, ref, low, sta = (new((H, n, D), dtype=q3.dtype, device=dev) for _ in range(5))
    mixed = new((H, n, D), dtype=q3.dtype, device=dev) if o3 is not None or precision is not None else None
    if n and sl["n_heads"]:
        keep_q, drop_q, keep_k = _coreset_lists(q3, k3, geom, hy, T, te, sl)  # as `routed_attention`'s coreset expert
        ops.gather_sample_rows(q3, tabs.rows, dst_q=q_own, dst_qrep=q_rep, dst_out=mixed if o3 is not None else None, out=o3, win=tabs.win,
                               keep_rows=keep_q, drop_rows=drop_q, **sl)
        n_low = geom.S_low + te
        dense = dict(k=k3, v=v3, scale=scale, **sl)  # the reference: the input dtype, whatever `precision`
        common = dense if precision is None else dict(_tier_key_side(precision, operands, q3, k3, v3, scale), scale=scale, **sl)
        full = dict(q=q_own, n_q=n, q_valid=n, n_kv=S + te, kv_rows=None if rm is None else rm[:S + te],
                    n_splits=fidelity_ref_splits(S + te))
        calls = [dict(dense, out=ref, tag="fidelity_ref", **full),
                 dict(common, q=q_rep, out=low, n_q=n, q_valid=n, n_kv=n_low, kv_rows=keep_k,
                      n_splits=fidelity_ref_splits(n_low), block_rows=SAMPLED_BLOCK_ROWS, tag="sampled_lowres")]
        if precision is not None:
            # (a fused grid is of one kernel family: the 16-bit reference goes alone, the tier's launches follow it)
            ops.attn_fwd_batch(calls[:1])
            calls = calls[1:] + [dict(common, out=mixed, tag="sampled_full", **full)]
        for start, count, lists, stride, n_kv, table, n_lists in tabs.classes:
            calls.append(dict(common, q=q_own[:, start:start + count], out=sta[:, start:start + count], n_q=count, n_kv=n_kv,
                              kv_rows=lists, kv_rows_stride_g=stride, q_block_table=table, n_key_lists=n_lists,
                              n_splits=fidelity_ref_splits(n_kv), block_rows=SAMPLED_BLOCK_ROWS, tag="sampled_sliding"))
        for i in range(0, len(calls), ops.MAX_FUSED):
            ops.attn_fwd_batch(calls[i:i + ops.MAX_FUSED])
    fid = ops.expert_fidelity([ref, low, sta], mixed)
    if sl["head_list"] is not None:  # NaN for the heads no slot names (slots at or past a device count are not read)
        count = sl["n_heads"] if sl["n_heads_dev"] is None else sl["n_heads_dev"]
        named = torch.zeros(H + 1, dtype=torch.bool, device=dev)
        named.index_fill_(0, _named_heads(torch.arange(sl["n_heads"], device=dev), count, sl["head_list"], H), True)
        named = named[:H]
        nan = lambda x: torch.where(named if x.dim() == 1 else named[:, None], x, torch.full_like(x, float("nan")))  # noqa: E731
        fid = fid._replace(sq_ref=nan(fid.sq_ref), max_ref=nan(fid.max_ref), sq_err=nan(fid.sq_err), max_err=nan(fid.max_err),
                           range_ref=nan(fid.range_ref))
    if outputs is not None:
        outputs.extend([ref, low, sta] + ([mixed] if mixed is not None else []) + [tabs.order])
    return fid


def _tier_key_side(precision: str, operands: Optional[AttnOperands], q3, k3, v3, scale) -> dict:
    """k, v and what goes with them of an 8-bit tier's launches, from `operands` of that precision or of "auto8" (whose int8
    launch is "i8pv"'s and whose 16-bit-score launch is "fp8pv"'s), prepared here where none is given"""
    if operands is None:
        operands = prepare_operands(precision, q3, k3, v3, scale)
    if operands.precision not in (precision, "auto8"):
        raise ValueError(f"sampled_expert_fidelity(precision={precision!r}): operands of {operands.precision!r}")
    kw = operands.tail_kwargs(scale) if (precision == "fp8pv" and operands.precision == "auto8") else operands.kwargs(scale)
    return {key: val for key, val in kw.items() if key not in ("q", "scale") and val is not None}


ROUTE_RULE_MODES = ("max_rel_error", "max_flops_share", "max_cost_share")
# the precision tiers a call may launch in, cheapest first, by the process precision (`set_attention_precision`); the last is
# where a head goes that no candidate serves.  Tier names and global ids: ops.TIER_NAMES (0 native, 1 fp8pv, 2 i8pv)
TIERS_OF_PRECISION = {"i8pv": ("i8pv", "native"), "fp8pv": ("fp8pv", "native"), "auto8": ("i8pv", "fp8pv", "native"),
                      "native": ("native",)}
DEFAULT_TIER_COST = ops.DEFAULT_TIER_COST  # (README.md: Wan-14B-81f, 1.25 x and 1.66 - 1.70 x the bf16 kernel)


def tiers_of(fp8=None) -> Tuple[str, ...]:
    """the tiers of an `fp8=` value (None: the process precision); "fp8" (both contractions in e4m3) is no product precision and
    has no tiers"""
    name = precision_of(fp8)
    if name not in TIERS_OF_PRECISION:
        raise ValueError(f"precision {name!r} has no tiers to route over: one of {tuple(TIERS_OF_PRECISION)}")
    return TIERS_OF_PRECISION[name]


@dataclass(frozen=True)
class RouteRule:
    """How the Eval processors route a call by its own measurement (`route_rule=`): `mode` one of ROUTE_RULE_MODES with its
    `value`, on `n_rows` sampled video rows per head (`sample_rows` with `seed`; every row where the clip has fewer).
    "max_cost_share" covers the precision by itself: it routes over the tiers of the process precision with or without
    `covers_precision`, under "native" over its one tier"""
    mode: str
    value: float
    n_rows: int = 512
    seed: int = 0
    # route over (precision tier, expert) pairs of the process precision: `tiers()` ("max_cost_share" always does)
    covers_precision: bool = False
    tier_cost: Optional[dict] = None     # tier -> cost of a FLOP there; None: DEFAULT_TIER_COST
    # verify what every call launched on the sampled rows and re-run the heads further than this from dense attention
    # (`routed_attention_repaired`); None: nothing is verified.  The patch layer reads it; `route()` does not
    repair_above: Optional[float] = None

    def __post_init__(self):
        if self.repair_above is not None and not float(self.repair_above) >= 0:
            raise ValueError(f"RouteRule: repair_above={self.repair_above} (a bound >= 0, or None)")
        if self.mode not in ROUTE_RULE_MODES or int(self.n_rows) < 1:
            raise ValueError(f"RouteRule: mode={self.mode!r} (one of {ROUTE_RULE_MODES}), n_rows={self.n_rows} (at least 1)")
        if self.covers_precision and self.mode == ROUTE_RULE_MODES[1]:
            raise ValueError("RouteRule: covers_precision goes with max_rel_error: max_flops_share has no form over precision "
                             "tiers (max_cost_share is the budget that has)")

    def tiers(self) -> Optional[Tuple[str, ...]]:
        """the tiers this rule routes over NOW, by the process precision; None where it routes experts alone -- without
        `covers_precision`, and under "native", whose one tier is the routes of today.  "max_cost_share" always routes over
        tiers: `tiers_of(None)`, ("native",) included"""
        if self.mode == ROUTE_RULE_MODES[2]:
            return tiers_of(None)
        if not self.covers_precision:
            return None
        tiers = tiers_of(None)
        return None if tiers == ("native",) else tiers

    def route(self, q, k, v, geom: "RoutedGeometry", **kw):
        """`route_by_fidelity` by this rule on (1,H,N,D) q, k, v: its 3-tuple, or its `TierRoutes` where `tiers()` names some"""
        rows = sample_rows(geom.S, min(int(self.n_rows), geom.S), int(self.seed), q.device)
        tiers = self.tiers()
        if tiers is not None:
            kw = dict(kw, tiers=tiers, tier_cost=self.tier_cost)
        return route_by_fidelity(q, k, v, geom, rows=rows, **{self.mode: float(self.value)}, **kw)


class TierRoutes(NamedTuple):
    """`route_by_fidelity(tiers=...)`: per tier, in the caller's order, the HeadRouting of its device lists; the int32 (H,)
    head -> expert and head -> GLOBAL tier id tables; per tier the record it was measured by; per 8-bit tier the operands
    that were prepared for the measurement (`routed_attention_tiers(operands=...)` launches with them); and the kernel's
    (n_tiers,3,H) lists and (n_tiers,3) counts the routings are views of; under `max_cost_share` also `level`, float32 (1,)
    on the device: the error the budget bought (None under the bound, which states its own)"""
    routings: Dict[str, "HeadRouting"]
    expert_ids: torch.Tensor
    tier_ids: torch.Tensor
    fids: Dict[str, "ops.ExpertFidelity"]
    operands: Dict[str, AttnOperands]
    lists: torch.Tensor
    counts: torch.Tensor
    level: Optional[torch.Tensor] = None


def route_by_fidelity(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, geom: RoutedGeometry, *, model: str,
                      text_len: int = 0, text_valid: int = 0, scale: Optional[float] = None, rows=None, seed: int = 0,
                      max_rel_error: Optional[float] = None, max_flops_share: Optional[float] = None,
                      tiers: Optional[Sequence] = None, tier_cost: Optional[dict] = None,
                      max_cost_share: Optional[float] = None):
    """Routes of one layer MEASURED on its own q, k, v, by a stated rule and without a router: `max_rel_error` = no sparse head
    may be further than that from dense attention on the sampled rows (per head the cheapest expert within the bound), or
    `max_flops_share` = spend at most that share of the dense layer's FLOPs where it hurts least (exactly one of the two;
    `vorta.patch.routes_from_fidelity` defines both).  Returns (HeadRouting, expert_ids, ops.ExpertFidelity): device head
    lists with device counts (`HeadRouting.from_device`), the int32 (H,) head -> expert table and the record they came from.
    Per call: `sampled_expert_fidelity` for every head with `out=None` (column 2 of the record stays NaN), then
    `ops.route_fidelity` with `work = expert_work(geom, text_valid, D)`.  Everything runs on the current stream, nothing is
    read back, graph-capturable once `geom.sample_tables` is built -- as the measurement is.
    Without `tiers` the measurement runs in the dtype of q, k, v whatever VORTA_ATTENTION_PRECISION says: the bound is on
    the METHOD (which keys a head sees) on the sampled rows, not on what an 8-bit precision adds to the routed launches.
    tiers: the precision tiers the call may launch in, cheapest first (names or global ids of ops.TIER_NAMES; `tiers_of()`
    gives the process precision's): the bound then covers the PRECISION too.  One measurement per tier -- `native`'s as
    above, an 8-bit tier's by `sampled_expert_fidelity(precision=tier)` on operands prepared once and handed on -- then
    `ops.route_fidelity_tiers` (`vorta.patch.routes_from_fidelity_tiers` is the rule: per head the cheapest (tier, expert)
    pair within the bound, cost = work[expert] * tier_cost[tier]; full attention in the last tier where none is).  Returns a
    `TierRoutes`; `routed_attention_tiers` launches it.  tier_cost: None = DEFAULT_TIER_COST.  `max_flops_share` with `tiers`
    is a ValueError by name.  What the bound covers: the candidate launches on the sampled rows, in each tier's own
    arithmetic; a full-size launch is that arithmetic with another key cut and, under "i8pv", another grouping of rows
    into waves.
    max_cost_share: the third rule, a budget that DOES cover the precision: spend at most that share of what the layer costs
    with every head on full attention in the last tier, on any expert in any tier, so that the largest per-head error is as
    small as that buys (`vorta.patch.routes_within_cost_share` is the rule; `ops.route_budget_tiers` applies it).  `tiers`
    None: `tiers_of(None)`, the process precision's -- under "native" its one tier.  The measurement per tier is the one
    above.  Always a `TierRoutes`, whose `level` is the error the budget bought.  With one tier this is not
    `max_flops_share`'s rule: that one gives a head one candidate, this one lets a head step down twice."""
    if tiers is not None and max_flops_share is not None:
        raise ValueError("route_by_fidelity: max_flops_share has no form over precision tiers; give max_rel_error")
    if sum(x is not None for x in (max_rel_error, max_flops_share, max_cost_share)) != 1:
        raise ValueError("route_by_fidelity: exactly one of max_rel_error and max_flops_share and max_cost_share")
    if max_cost_share is not None:
        if isinstance(max_cost_share, (bool, str)) or not float(max_cost_share) > 0:
            raise ValueError(f"route_by_fidelity: max_cost_share={max_cost_share!r} (a positive share)")
        if tiers is None:
            tiers = tiers_of(None)
    if rows is not None and (rows.numel() if torch.is_tensor(rows) else int(rows)) < 1:
        raise ValueError("route_by_fidelity: rows: at least one sampled row (without one every error reads 0 and every head "
                         "would meet any bound)")
    from .patch.fidelity import expert_work
    fid = sampled_expert_fidelity(q, k, v, geom, model=model, text_len=text_len, text_valid=text_valid, scale=scale, rows=rows,
                                  seed=seed)
    work = expert_work(geom, text_valid if model == "hunyuan" else 0, q.shape[-1])
    if tiers is not None:
        rule = dict(max_rel_error=float(max_rel_error)) if max_cost_share is None else dict(max_cost_share=float(max_cost_share))
        return _route_tiers(q, k, v, geom, fid, work, tiers, tier_cost, rule,
                            dict(model=model, text_len=text_len, text_valid=text_valid, scale=scale, rows=rows, seed=seed))
    expert, lists, counts = ops.route_fidelity(fid, max_rel_error=max_rel_error, max_flops_share=max_flops_share, work=work)
    return HeadRouting.from_device(lists, counts), expert, fid


def _route_tiers(q, k, v, geom, native_fid, work, tiers, tier_cost, rule: dict, measure_kw: dict) -> TierRoutes:
    """`route_by_fidelity(tiers=...)` after the native measurement; `rule`: max_rel_error or max_cost_share with its value"""
    names = [ops.TIER_NAMES[ops.tier_id(t)] for t in tiers]
    q3, k3, v3 = _fold(q), _fold(k), _fold(v)
    operands: Dict[str, AttnOperands] = {}
    if "i8pv" in names:
        operands["i8pv"] = prepare_operands("i8pv", q3, k3, v3, measure_kw["scale"])
    if "fp8pv" in names:  # (the e4m3 V of "i8pv" is "fp8pv"'s: one conversion serves both)
        i8 = operands.get("i8pv")
        operands["fp8pv"] = (prepare_operands("fp8pv", q3, k3, v3, measure_kw["scale"]) if i8 is None
                             else AttnOperands("fp8pv", q3, k3, i8.v, i8.v_descale))
    fids = {name: native_fid if name == "native" else
            sampled_expert_fidelity(q, k, v, geom, precision=name, operands=operands[name], **measure_kw) for name in names}
    level = None
    if "max_cost_share" in rule:
        expert, tier, lists, counts, level = ops.route_budget_tiers(fids, work=work, tier_cost=tier_cost, **rule)
    else:
        expert, tier, lists, counts = ops.route_fidelity_tiers(fids, work=work, tier_cost=tier_cost, **rule)
    tier_ids = torch.zeros_like(tier)
    for i, name in enumerate(names):  # the caller's index -> the global id, on the device
        tier_ids = torch.where(tier == i, ops.TIER_NAMES.index(name), tier_ids)
    routings = {name: HeadRouting.from_device(lists[i], counts[i]) for i, name in enumerate(names)}
    return TierRoutes(routings, expert, tier_ids, fids, operands, lists, counts, level)


def tier_sink_entry(routes: TierRoutes) -> tuple:
    """what a processor's `route_sink` receives for a call routed over tiers: the four entries of a call routed over experts
    -- expert_ids, lists (n_tiers,3,H), counts (n_tiers,3), a record (`native`'s, the method's error, where that tier is one of
    them; else the first tier's) -- and the tier data, `level` included (None under the bound)"""
    fid = routes.fids.get("native", next(iter(routes.fids.values())))
    return (routes.expert_ids, routes.lists, routes.counts, fid,
            dict(tiers=tuple(routes.routings), tier_ids=routes.tier_ids, fids=routes.fids, level=routes.level))


def _merge_sampled(records) -> "ops.SampledFidelity":
    """the per-tier records of one `routed_attention_tiers` call as one: every head from the record that measured it"""
    first = records[0]
    for other in records[1:]:
        pick = lambda a, b: None if a is None or b is None else torch.where(torch.isnan(a), b, a)  # noqa: E731
        expert = None if first.expert is None or other.expert is None else torch.where(first.expert < 0, other.expert, first.expert)
        first = first._replace(sq_ref=pick(first.sq_ref, other.sq_ref), max_ref=pick(first.max_ref, other.max_ref),
                               sq_err=pick(first.sq_err, other.sq_err), max_err=pick(first.max_err, other.max_err),
                               range_ref=pick(first.range_ref, other.range_ref),
                               row_sq_err=pick(first.row_sq_err, other.row_sq_err), expert=expert)
    return first


def _launch_tiers(q, k, v, routings, geom, operands, records: Optional[list], heads_of=None, **kw) -> None:
    """one `routed_attention` call per tier of `routings`, in their order: `fp8=` the tier (False for `native`), the tier's
    entry of `operands`, `records` the fidelity sink of every call (None: none measures); heads_of: tier name -> its
    `fidelity_heads` (None: the caller's keyword, if any)"""
    for tier, routing in routings.items():
        name = ops.TIER_NAMES[ops.tier_id(tier)]
        if heads_of is not None:
            kw["fidelity_heads"] = heads_of(name)
        routed_attention(q, k, v, routing, geom, fp8=False if name == "native" else name,
                         operands=None if operands is None else operands.get(name), fidelity=records, **kw)


def routed_attention_tiers(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routings, geom: RoutedGeometry, *,
                           out: Optional[torch.Tensor] = None, operands: Optional[Dict[str, AttnOperands]] = None,
                           fidelity: Optional[list] = None, **kw) -> torch.Tensor:
    """One `routed_attention` call per precision tier: `routings` maps a tier (a name or global id of ops.TIER_NAMES) to the
    HeadRouting of the heads that run in it (`TierRoutes.routings`; a head is in one list of one tier), each with `fp8=` that
    tier, all writing disjoint heads of one `out`.  A tier whose device lists are empty launches workgroups that exit at once,
    as "auto8"'s second part does.  operands: tier -> AttnOperands prepared already (`TierRoutes.operands`); a tier without
    an entry converts its own.  fidelity: receives ONE `ops.SampledFidelity`, every head from the call that launched it.
    Other keywords go to every `routed_attention` call (`fp8`, `fp8_operands`, `expert_outs` do not apply)."""
    for bad in ("fp8", "fp8_operands", "expert_outs", "expert_fidelity"):
        if bad in kw:
            raise ValueError(f"routed_attention_tiers: {bad}= does not apply: a tier names its precision, one `out` takes the heads")
    if out is None:
        out = torch.empty_like(q)
    records: list = []
    _launch_tiers(q, k, v, routings, geom, operands, None if fidelity is None else records, out=out, **kw)
    if fidelity is not None:
        fidelity.append(_merge_sampled(records))
    return out


def _side_streams(device: torch.device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _SIDE_STREAMS:
        _SIDE_STREAMS[idx] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
    return _SIDE_STREAMS[idx]


def routed_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routing: HeadRouting,
                     geom: RoutedGeometry, *, model: str, text_len: int = 0, text_valid: int = 0,
                     out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                     concurrent: bool = False, fused: bool = True, sliding_block_rows: int = 0,
                     expert_outs: Optional[Sequence[torch.Tensor]] = None, fp8=None, fp8_operands=None,
                     operands: Optional[AttnOperands] = None, kv_splits: int = 1,
                     record: Optional[list] = None, fidelity: Optional[list] = None, fidelity_rows=None,
                     fidelity_heads: str = "sparse", expert_fidelity: Optional[list] = None) -> torch.Tensor:
    """q,k,v: (1,H,S+T,D) [hunyuan: video then text] or (1,H,S,D) [wan].  Returns (1,H,S+T,D).

    hunyuan: hunyuan.py:556-605 (TripleEval.__call__ steps 5.1-5.4);  wan: wan.py:351-383.

    fused=True (default) submits the experts' attention launches as ONE grid (vorta_attn_fwd_batch): workgroups of
    the full expert first, then coreset, then sliding tile, so each expert's tail is filled by the next one.
    concurrent=True instead enqueues the coreset and sliding-tile experts on two side HIP streams (forked from and joined
    back into the current stream with events): the experts are independent, so the tail of one launch (a few
    hundred workgroups on 256 CUs when only H/P heads are local) is filled by the next expert's workgroups.
    expert_outs: one output tensor per expert instead of `out` (heads may then appear under several experts).
    fp8=True: both contractions in e4m3 (BASELINE.json configs[4]; no reference counterpart): q,k,v are converted once
    per call (`prepare_operands`, `fp8_operands` to reuse buffers) and every expert launch reads the e4m3 copies; the
    coreset ranking still reads the 16-bit q/k (coreset_select.py:98-105 ranks in the input dtype).  Other values:
    `precision_of`; fp8=None follows the process-wide default (`set_attention_precision`, VORTA_ATTENTION_PRECISION).
    operands: AttnOperands with the geometry of q,k,v prepared elsewhere (the sequence-parallel path converts the receive
    buffers once, vorta_amd/ulysses/engine.py RecvOperands); `fp8` and `fp8_operands` are then not read.
    kv_splits > 1: the full-attention and coreset launches cut their KEYS into that many parts (+ a merge kernel) -- for
    a sequence-parallel rank whose one or two heads leave the chip under one round of workgroups, where a layer lasts as
    long as one workgroup's key loop; changes the summation order, so it is never chosen silently.
    record: a list that receives the launches as launched -- the dictionaries of ops.attn_fwd keywords (q / k / v / out,
    tables, head lists, lengths), in launch order; the backward replays them through ops.attn_bwd (`_replay_backward`).
    fidelity: a list that receives one `ops.SampledFidelity` of this call: after the routed launches, dense attention in the
    input dtype (the ORIGINAL 16-bit q, k, v, whatever the precision) on `fidelity_rows` sampled video rows per head -- a
    sample size (None: min(DEFAULT_FIDELITY_ROWS, S); `sample_rows` with seed 0) or an int32 table of `sample_rows` -- against
    the rows this call wrote, per head, as run: hard routes, 8-bit precision, partial geometry, a rank's local heads.
    fidelity_heads: "sparse" = the heads of experts 1 and 2, "all" = expert 0's as well (what 8 bits cost a full head); heads
    split by query range are never measured; unmeasured heads hold NaN.  Every launch is on the current stream, nothing is
    read back (the record's `expert` ids are a device tensor).  None (default): nothing is allocated or launched beyond the
    routed calls; `out` has the same bits either way.  The reference launches are launches of their own after the routed grid.
    expert_fidelity: a list that receives one `ops.ExpertFidelity` of this call: `sampled_expert_fidelity` on the same
    `fidelity_rows`, for every head, after the routed launches and with `out=` this call's output -- what each expert WOULD
    have written on the sampled rows (columns 0 / 1) beside what the call did write (column 2), all against dense attention
    in the input dtype.  None (default): nothing is allocated or launched for it."""
    if q.dim() == 4 and q.shape[0] != 1:
        # hunyuan.py:168 asserts batch 1; Wan's CFG runs two batch-1 forwards (pipeline_wan.py:322-344)
        raise AssertionError(f"Batch size {q.shape[0]} is not supported by routed_attention.")
    hy = model == "hunyuan"
    H, N, D = q.shape[-3], q.shape[-2], q.shape[-1]
    S, T = geom.S, (text_len if hy else 0)
    rm = geom.row_map
    if rm is None and N != S + T:
        raise ValueError(f"Input sequence length {N - T} does not match latent shape {geom.latent}.")
    te = text_valid if hy else 0
    if (fidelity is not None or expert_fidelity is not None) and expert_outs is not None:
        raise ValueError("fidelity= / expert_fidelity= measure the routed output `out`: they do not go with expert_outs")
    if out is None and expert_outs is None:
        out = torch.empty_like(q)
    q3, k3, v3 = _fold(q), _fold(k), _fold(v)
    o_e = [_fold(out)] * 3 if expert_outs is None else [_fold(x) for x in expert_outs]

    def live(e):
        return routing.counts_host is None or routing.counts_host[e] > 0 or (e == 0 and bool(routing.partials))

    def nheads(e):  # for the algorithmic-work tags only
        return routing.counts_host[e] if routing.counts_host is not None else 0

    if operands is None:
        # (video_tokens: the sample is summed in eighths of the video tokens + the text, as the sequence-parallel send side sums it)
        operands = prepare_operands(precision_of(fp8), q3, k3, v3, scale, fp8_operands,
                                    video_tokens=S if rm is None and T > 0 else 0)
    split_kw = dict(n_splits=int(kv_splits)) if kv_splits and int(kv_splits) > 1 else {}
    # one pass of the experts' launches: (base, slot_of, slot_part) -- the operands' keywords; (expert, H) -> head_list / n_heads /
    # n_heads_dev of a launch; the same for part i of a head split by query range.  "auto8" makes two passes (below)
    passes = [(operands.kwargs(scale), routing.slot_args, lambda i, hl: dict(head_list=hl, n_heads=1, n_heads_dev=None))]

    # ---- expert 0: full attention (hunyuan.py:136-189 / wan.py:142-145) ----
    def expert_full(base, slot_of, slot_part):
        calls = []
        if routing.counts_host is None or routing.counts_host[0] > 0:
            calls.append(dict(base, out=o_e[0], tag="full", **_full_launch(geom, T, te, kv_splits),
                              flops=nheads(0) * 4.0 * (S + te) ** 2 * D, **slot_of(0, H)))
        for pi, (hl, t0, t1) in enumerate(routing.partials or ()):
            # a head whose other query tokens another rank computes: every key, the query rows [t0, t1) of the VIDEO tokens;
            # the part that ends at the last video token also owns the head's text queries (they follow it in token order)
            if not (0 <= t0 < t1 <= S):
                raise ValueError(f"query range [{t0}, {t1}) outside the {S} video tokens")
            e1, v1 = (S + T, S + te) if (t1 == S and T > 0) else (t1, t1)
            part = dict(base, out=o_e[0], n_q=e1 - t0, n_kv=S + te, q_valid=v1 - t0, tag="full_part", **split_kw,
                        kv_rows=None if rm is None else rm[:S + te], flops=4.0 * (v1 - t0) * (S + te) * D,
                        **slot_part(pi, hl))
            if rm is None:
                part.update(q_row_offset=t0)
            else:
                part.update(q_rows=rm[t0:e1])
            calls.append(part)
        return calls

    # ---- expert 1: coreset attention (hunyuan.py:410-457 / wan.py:243-270) ----
    def expert_lowres(base, slot_of, slot_part):
        sl = slot_of(1, H)
        keep_q, drop_q, keep_k = _coreset_lists(q3, k3, geom, hy, T, te, sl)
        return [dict(base, out=o_e[1], n_q=geom.S_low + T, n_kv=geom.S_low + te, q_valid=geom.S_low + te, q_rows=keep_q,
                     kv_rows=keep_k, dup_rows=drop_q, n_dup_pos=geom.G, tag="lowres", **split_kw,
                     flops=nheads(1) * 4.0 * (geom.S_low + te) ** 2 * D, **sl)]

    # ---- expert 2: sliding-tile attention (hunyuan.py:459-507 / wan.py:272-294) ----
    def expert_sliding(base, slot_of, slot_part):
        sl = slot_of(2, H)
        if geom.is_partial:
            # always the merged form, one launch per key-list length (RoutedGeometry.sta_partial_launches)
            br = sliding_block_rows if sliding_block_rows in (128, 256) else 256
            calls = [dict(base, out=o_e[2], n_q=q_rows.numel(), n_kv=n_kv, q_rows=q_rows, kv_rows=kv_rows,
                          kv_rows_stride_g=stride, q_block_table=table, n_key_lists=n_lists, tag="sliding",
                          flops=nheads(2) * 4.0 * D * q_rows.numel() * n_kv, block_rows=br, **sl)
                     for q_rows, kv_rows, stride, n_kv, table, n_lists in geom.sta_partial_launches(te, br)]
        elif STA_MERGE and sliding_block_rows in (128, 256):
            q_rows, kv_rows, n_kv, table, n_lists = geom.sta_launch_tables(te, sliding_block_rows)
            calls = [dict(base, out=o_e[2], n_q=S, n_kv=n_kv, q_rows=q_rows, kv_rows=kv_rows, kv_rows_stride_g=n_kv,
                          q_block_table=table, n_key_lists=n_lists, tag="sliding", flops=nheads(2) * 4.0 * D * S * n_kv,
                          block_rows=sliding_block_rows, **sl)]
        else:
            q_rows, kv_rows, n_kv = geom.sta_tables(te)
            calls = [dict(base, out=o_e[2], n_q=S, q_group_len=geom.tok, n_kv=n_kv, q_rows=q_rows, kv_rows=kv_rows,
                          kv_rows_stride_g=n_kv, tag="sliding", flops=nheads(2) * 4.0 * D * S * n_kv,
                          block_rows=sliding_block_rows, **sl)]
        if T > 0:
            # text queries see every valid key (sliding_attn_flex.py:108); padded ones see nothing -> zeros
            txt = dict(base, out=o_e[2], n_q=T, q_valid=te, n_kv=S + te, n_splits=_auto_splits(sl["n_heads"], T, S + te),
                       tag="sliding_text", flops=nheads(2) * 4.0 * D * te * (S + te), **sl)
            if FUSED_TEXT_FIRST:
                # hints for ops.attn_fwd_batch, honoured only if this call joins a fused grid: there the one query block
                # per head need not fill the chip, only not be the grid's tail -- dispatched FIRST and unsplit it is as
                # long as a full-attention workgroup, with no partials to write and no combine launch.  A stand-alone
                # launch (T not a multiple of 256, variant 1, ...) keeps the 64-232 key splits above.  Measured on one
                # box, splits 0(last, auto) / 8 / 4 / 2 / 1: rank of 8 549.5 / 542.2 / 540.0 | 557.0 (4) / 553.9 / 552.8 ms;
                # one GPU 4 130 / 4 115 (8) | 4 226 (4) / 4 208 (1)
                txt.update(fused_n_splits=FUSED_TEXT_SPLITS, fused_first=True)
            if rm is None:
                txt.update(q_row_offset=S)
            else:
                txt.update(q_rows=rm[S:S + T], kv_rows=rm[:S + te])
            calls.append(txt)
        return calls

    def launch_fused(calls):
        # a partial geometry may bring more launches than one grid takes (up to eight sliding classes): consecutive fused
        # grids in list order.  Every launch writes rows of its own, so the grouping does not show in the result
        if record is not None:
            record.extend(calls)
        for i in range(0, max(len(calls), 1), ops.MAX_FUSED):
            ops.attn_fwd_batch(calls[i:i + ops.MAX_FUSED])

    def launch(calls):
        if record is not None:
            record.extend(calls)
        for c in calls:
            c = {key: val for key, val in c.items() if key not in ("fused_n_splits", "fused_first")}
            ops.attn_fwd(c.pop("q"), c.pop("k"), c.pop("v"), c.pop("out"), **c)

    def measured(result):
        if fidelity is not None:
            _measure_routed(fidelity, fidelity_rows, fidelity_heads, q3, k3, v3, o_e[0], routing, geom, te, scale)
        if expert_fidelity is not None:
            expert_fidelity.append(sampled_expert_fidelity(q3, k3, v3, geom, model=model, text_len=T, text_valid=te, scale=scale,
                                                           rows=fidelity_rows, out=o_e[0]))
        return result

    if fused and not concurrent and sliding_block_rows == 0:
        # 256-row workgroups let the sliding launch join the fused grid; measured better than a separate
        # 128-row launch with less padding (Hunyuan 129f: 4.77 s vs 4.91 s per step)
        sliding_block_rows = 256
    experts = [(expert_full, live(0)), (expert_lowres, live(1)), (expert_sliding, live(2))]
    if operands.precision == "auto8":
        if concurrent:
            raise ValueError("'auto8' runs its two parts as fused grids (concurrent=False)")
        parts = [ops.split_heads(operands.tail, **routing.slot_args(e, H)) if on else None for e, (_, on) in enumerate(experts)]
        pparts = [ops.split_heads(operands.tail, hl, 1) for hl, _, _ in routing.partials or ()]
        passes = [(b, lambda e, H_, which=which: parts[e][which], lambda i, hl, which=which: pparts[i][which])
                  for which, b in ((0, passes[0][0]), (1, operands.tail_kwargs(scale)))]  # int8-score heads, then 16-bit-score heads
    if not concurrent:
        for one in passes:
            calls = [c for fn, on in experts if on for c in fn(*one)]
            if fused:
                launch_fused(calls)
            else:
                launch(calls)
        return measured(out)
    # the experts are independent: fork them onto side streams, join before returning (so every later use of
    # q,k,v,out on the current stream is ordered after them)
    cur = torch.cuda.current_stream(q.device)
    fork = torch.cuda.Event()
    fork.record(cur)
    streams = (None,) + _side_streams(q.device)
    for (fn, on), st in zip(experts, streams):
        if not on:
            continue
        if st is None:
            launch(fn(*passes[0]))
            continue
        st.wait_event(fork)
        with torch.cuda.stream(st):
            launch(fn(*passes[0]))
            done = torch.cuda.Event()
            done.record(st)
        cur.wait_event(done)
    return measured(out)


@dataclass(eq=False)
class RepairableRoutes:
    """The device route tables of one layer in the form `routed_attention_repaired` verifies and vorta_route_repair rewrites
    IN PLACE: the tiers' names in launch order, the int32 head -> expert (H,) and head -> tier INDEX (H,; None with the single
    tier) tables, and the contiguous (n_tiers,3,H) lists and (n_tiers,3) counts the launches read.  `routings` are views of
    the lists and counts: a repair shows in the next launch, and in a captured graph's replay."""
    tiers: Tuple[str, ...]
    expert_ids: torch.Tensor
    tier_index: Optional[torch.Tensor]
    lists: torch.Tensor
    counts: torch.Tensor
    tier_ids: Optional[torch.Tensor] = None              # a `TierRoutes`' GLOBAL ids: kept in step with `tier_index`

    @property
    def routings(self) -> Dict[str, "HeadRouting"]:
        return {name: HeadRouting.from_device(self.lists[i], self.counts[i]) for i, name in enumerate(self.tiers)}

    @staticmethod
    def from_routes(routes, precision: str = "native") -> "RepairableRoutes":
        """of a `TierRoutes`, of a (HeadRouting.from_device, expert_ids) pair under the single `native` tier (a HeadRouting
        that carries its `expert_ids` goes alone), or of a RepairableRoutes (itself).  `precision`: the precision a single
        routing would be launched in: an 8-bit one is refused by name (a bound on what is launched has to route over what is
        launched)."""
        if isinstance(routes, RepairableRoutes):
            made = routes
        elif isinstance(routes, TierRoutes):
            names = tuple(ops.TIER_NAMES[ops.tier_id(t)] for t in routes.routings)
            index = torch.zeros_like(routes.tier_ids)
            for i, name in enumerate(names):  # the global id -> the caller's index, on the device
                index = torch.where(routes.tier_ids == ops.TIER_NAMES.index(name), i, index)
            made = RepairableRoutes(names, routes.expert_ids, index.to(torch.int32), routes.lists, routes.counts,
                                    routes.tier_ids)
        else:
            routing = expert_ids = None
            if isinstance(routes, HeadRouting):
                routing, expert_ids = routes, routes.expert_ids
                if expert_ids is None and routes.counts_dev is not None:  # (derived from the lists, on the device)
                    expert_ids = _expert_ids(routes, routes.lists.shape[-1], routes.lists.device)
            elif isinstance(routes, (tuple, list)) and len(routes) == 2:
                routing, expert_ids = routes
            if not isinstance(routing, HeadRouting) or not torch.is_tensor(expert_ids):
                raise ValueError("routed_attention_repaired: routes are a TierRoutes, a RepairableRoutes or a "
                                 "(HeadRouting.from_device(lists, counts), expert_ids) pair")
            if routing.counts_dev is None or routing.partials:
                raise ValueError("routed_attention_repaired: the routes are repaired on the device: a HeadRouting.from_device "
                                 "(device counts, no heads split by query range)")
            H = expert_ids.numel()
            made = RepairableRoutes(("native",), expert_ids, None, routing.lists.view(1, 3, H), routing.counts_dev.view(1, 3))
        if made.tier_index is None and precision != "native":
            raise ValueError(f"routed_attention_repaired: under the 8-bit precision {precision!r} the routes must be tier "
                             "routes (measured_routes(covers_precision=True), route_by_fidelity(tiers=...) or "
                             "fixed_routes(precisions=...)): 'auto8' is not a tier name, and a bound on what is launched has "
                             "to route over what is launched")
        if "native" not in made.tiers:
            raise ValueError(f"routed_attention_repaired: the tiers {made.tiers} must include 'native': a repaired head runs full "
                             "attention in the input dtype")
        return made


class RepairRecord(NamedTuple):
    """`routed_attention_repaired`: what was verified and what was done about it, all on the device"""
    fidelity: "ops.SampledFidelity"   # the rows AS LAUNCHED, before the repair
    state_of_head: torch.Tensor       # int32 (H,): 0 not checked, 1 kept, 2 repaired
    rel: torch.Tensor                 # float32 (H,): the error as checked, NaN for a head that was not checked
    repair_list: torch.Tensor         # int32 (H,): the heads repaired by this call, ascending; entries past the count unwritten
    repair_count: torch.Tensor        # int32 (1,)
    routes: Optional[RepairableRoutes] = None   # the tables the call verified, as they stand after the repair


def routed_attention_repaired(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routes, geom: RoutedGeometry, *,
                              repair_above: Optional[float], rows=None, model: str, text_len: int = 0, text_valid: int = 0,
                              out: Optional[torch.Tensor] = None, scale: Optional[float] = None, fp8=None,
                              operands: Optional[Dict[str, AttnOperands]] = None, record: Optional[list] = None,
                              **kw) -> Tuple[torch.Tensor, Optional[RepairRecord]]:
    """A routed call that VERIFIES what it launched on sampled rows and re-runs the heads over a stated error, in one forward
    and without a host read.  `routes`: a `TierRoutes`, a `RepairableRoutes`, or a (HeadRouting.from_device, expert_ids) pair,
    which runs under the single `native` tier.  `rows`: the sampled video rows, as `routed_attention(fidelity_rows=...)`.
    operands: tier -> AttnOperands prepared already FOR THESE q, k, v (`TierRoutes.operands` of a measurement on them), as
    `routed_attention_tiers` takes them.
    (a) The routings are launched as `routed_attention_tiers` / `routed_attention` launch them, with a fidelity sink on
    `rows`.  A head whose launch is the reference itself -- full attention in the input dtype -- is not measured: the native
    tier measures its sparse heads, an 8-bit tier every head.  (b) `ops.route_repair` on that record: a checked head with
    rel > repair_above (or NaN) becomes (expert 0, native) in the route tables, IN PLACE -- later calls with the same tables
    launch it dense.  (c) One dense launch in the input dtype over the repaired heads, with the device count, writes them into
    the same `out`: the arguments of `routed_attention`'s expert 0, Hunyuan's text rows included; no coreset selection runs
    for it, and with a zero count its workgroups exit at once.
    Returns (out, RepairRecord).  On the sampled rows no head leaves the call further than `repair_above` from dense
    attention; the repaired heads are dense launches with their own key cut.  Graph-capturable once the geometry's tables are
    built.  `repair_above=None`: the routings are launched as today, nothing more; returns (out, None).
    ValueError by name for tiers without `native`, for a single routing under an 8-bit precision (`fp8`; None: the process
    precision), and for a negative or NaN bound."""
    if repair_above is not None and not float(repair_above) >= 0:
        raise ValueError(f"routed_attention_repaired: repair_above={repair_above} (a bound >= 0, or None)")
    rr = RepairableRoutes.from_routes(routes, "native" if repair_above is None else precision_of(fp8))
    if out is None:
        out = torch.empty_like(q)
    common = dict(model=model, text_len=text_len, text_valid=text_valid, out=out, scale=scale, record=record, **kw)
    single = rr.tier_index is None
    if repair_above is None:
        if single:
            routed_attention(q, k, v, HeadRouting.from_device(rr.lists[0], rr.counts[0]), geom, fp8=fp8, **common)
        else:
            routed_attention_tiers(q, k, v, rr.routings, geom, operands=operands, **common)
        return out, None
    records: list = []
    _launch_tiers(q, k, v, rr.routings, geom, operands, records, lambda name: "sparse" if name == "native" else "all",
                  fidelity_rows=rows, **common)
    fid = _merge_sampled(records)
    exact = rr.tiers.index("native")
    repair_list, repair_count, state, rel = ops.route_repair(fid.sq_ref, fid.sq_err, rr.expert_ids, rr.tier_index, rr.lists,
                                                             rr.counts, exact_tier=exact, repair_above=float(repair_above))
    if rr.tier_ids is not None:  # (a TierRoutes' global ids follow: every repaired head is in `native` now)
        rr.tier_ids.masked_fill_(state == 2, ops.TIER_NAMES.index("native"))
    T, te = (text_len, text_valid) if model == "hunyuan" else (0, 0)
    dense = dict(q=_fold(q), k=_fold(k), v=_fold(v), scale=scale, out=_fold(out), tag="repair", flops=0.0,
                 head_list=repair_list, n_heads=q.shape[-3], n_heads_dev=repair_count,
                 **_full_launch(geom, T, te, kw.get("kv_splits")))
    if record is not None:
        record.append(dense)
    ops.attn_fwd_batch([dense])
    return out, RepairRecord(fid, state, rel, repair_list, repair_count, rr)


def soft_mixture_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routing_score: torch.Tensor,
                           geom: RoutedGeometry, *, model: str, text_len: int = 0, text_valid: int = 0,
                           out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                           fidelity: Optional[list] = None) -> torch.Tensor:
    """Training-time FORWARD: every head through all three experts, outputs mixed with the routing
    scores of batch item 0 -- hunyuan.py:375-408,509-513 / wan.py:226-241,296-300.  The three experts over all H
    heads run as one fused grid into three buffers; `vorta_mix_experts` does the weighted sum in one pass.
    No autograd: the library has no backward kernels (router training itself is out of scope).
    (The differentiable form of this operator is `soft_mixture_attention_autograd`, below.)
    fidelity: a list that receives one `ops.ExpertFidelity` of this call's H heads (one more pass over the three expert
    outputs and the mixed output, ops.expert_fidelity); None (default): the launches and the bits of `out` are unchanged."""
    H = q.shape[-3]
    if out is None:
        out = torch.empty_like(q)
    bufs = [torch.empty_like(out) for _ in range(3)]
    # fp8=False: the training-time forward feeds a loss; the e4m3 switch is an inference-time option of the routed op
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, q.device), geom, model=model, text_len=text_len,
                     text_valid=text_valid, scale=scale, expert_outs=bufs, fp8=False)
    ops.mix_experts([b[0] if b.dim() == 4 else b for b in bufs], routing_score, out[0] if out.dim() == 4 else out)
    if fidelity is not None:
        fidelity.append(ops.expert_fidelity(bufs, out))
    return out


ATTENTION_BACKWARDS = ("query_major", "key_major", "deterministic")
_attention_backward = None  # the process-wide default; None = not set: VORTA_ATTENTION_BACKWARD, else "query_major"


def _check_backward(name: str, where: str) -> str:
    if name not in ATTENTION_BACKWARDS:
        raise ValueError(f"{where}: unknown attention backward {name!r} (one of {', '.join(ATTENTION_BACKWARDS)})")
    return name


def set_attention_backward(name: str) -> None:
    """the process-wide attention backward algorithm of the differentiable operators and processors: "query_major"
    (ops.attn_bwd: dq bit-reproducible), "key_major" (ops.attn_bwd_stats + ops.attn_bwd_key_major: a quarter of the atomic
    bytes, nothing bit-reproducible) or "deterministic" (ops.attn_bwd_stats + ops.attn_bwd_dq + ops.attn_bwd_dkv: no atomics,
    dq, dk and dv bit-reproducible).  Overrides the environment switch VORTA_ATTENTION_BACKWARD.  This switch is the only
    selector: torch.use_deterministic_algorithms is not consulted.  It holds on one GPU and under sequence parallelism alike
    (`sp_soft_mixture_attention_autograd`, the Train processors' sequence-parallel grad mode): an operator reads it when its
    forward runs.  Under sequence parallelism "deterministic" makes every RANK's gradients repeat bit for bit; what a training
    loop sums across ranks afterwards (text-row and score gradients) is that loop's own order."""
    global _attention_backward
    _attention_backward = _check_backward(name, "set_attention_backward")


def attention_backward(backward: Optional[str] = None) -> str:
    """the algorithm a call with `backward` uses: its own choice, else set_attention_backward's, else the environment's
    VORTA_ATTENTION_BACKWARD, else "query_major" """
    if backward is not None:
        return _check_backward(backward, "backward")
    if _attention_backward is not None:
        return _attention_backward
    import os
    return _check_backward(os.environ.get("VORTA_ATTENTION_BACKWARD") or "query_major", "VORTA_ATTENTION_BACKWARD")


def _attn_bwd_by(algorithm: str, q, k, v, o, d_out, dq, dk, dv, do_scale=None, **launch) -> None:
    """the gradient of one recorded launch by one of ATTENTION_BACKWARDS"""
    if algorithm == "key_major":
        stats = ops.attn_bwd_stats(q, k, v, o, d_out, do_scale=do_scale, **launch)
        ops.attn_bwd_key_major(q, k, v, o, d_out, dq, dk, dv, stats, do_scale=do_scale, **launch)
    elif algorithm == "deterministic":
        stats = ops.attn_bwd_stats(q, k, v, o, d_out, do_scale=do_scale, **launch)
        ops.attn_bwd_dq(q, k, v, o, d_out, dq, stats, do_scale=do_scale, **launch)
        ops.attn_bwd_dkv(q, k, v, o, d_out, dk, dv, stats, do_scale=do_scale, **launch)
    else:
        ops.attn_bwd(q, k, v, o, d_out, dq, dk, dv, do_scale=do_scale, **launch)


def _replay_backward(launches, d_out: torch.Tensor, dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor,
                     weight_of=None, algorithm: str = "query_major") -> None:
    """one backward per recorded forward launch, with the SAME dictionaries (forward and backward cannot disagree on a
    table): ops.attn_bwd ("query_major"), the statistics pass and then the key-major pass ("key_major"), or the statistics
    pass, the dQ pass and the dK / dV pass ("deterministic");
    `weight_of(launch, out)` = the per-head weight of the launch's output in the loss (None: 1)"""
    _check_backward(algorithm, "_replay_backward")
    for c in launches:
        c = dict(c)
        q, k, v, o = c.pop("q"), c.pop("k"), c.pop("v"), c.pop("out")
        _attn_bwd_by(algorithm, q, k, v, o, d_out, dq, dk, dv, do_scale=None if weight_of is None else weight_of(c, o), **c)


def _unbind_launches(launches, outs) -> list:
    """the recorded launches without q / k / v / out; `expert` keeps which of `outs` a launch wrote.  An autograd node keeps
    these beside its SAVED q, k, v and expert outputs and binds them again in its backward (`_bind_launches`): inside a
    checkpointed region the saved tensors are the recomputed ones and the forward's own are gone (and must not be kept
    alive by the dictionaries).  The tables stay: constants of the backward, equal in a recompute."""
    ptrs = [o.data_ptr() for o in outs]
    return [dict({n: x for n, x in c.items() if n not in ("q", "k", "v", "out")}, expert=ptrs.index(c["out"].data_ptr()))
            for c in launches]


def _bind_launches(launches, q, k, v, outs) -> list:
    return [dict({n: x for n, x in c.items() if n != "expert"}, q=q, k=k, v=v, out=outs[c["expert"]]) for c in launches]


class _SoftMixture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, routing_score, geom, model, text_len, text_valid, scale, backward, fidelity=None):
        ctx.algorithm = attention_backward(backward)
        H = q.shape[-3]
        out = torch.empty_like(q)
        bufs = [torch.empty_like(out) for _ in range(3)]
        launches: list = []
        routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, q.device), geom, model=model, text_len=text_len,
                         text_valid=text_valid, scale=scale, expert_outs=bufs, fp8=False, record=launches)
        ops.mix_experts([b[0] if b.dim() == 4 else b for b in bufs], routing_score, out[0] if out.dim() == 4 else out)
        if fidelity is not None:
            fidelity.append(ops.expert_fidelity(bufs, out))
        ctx.save_for_backward(q, k, v, routing_score, *bufs)
        ctx.launches = _unbind_launches(launches, [b[0] if b.dim() == 4 else b for b in bufs])
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, routing_score, *bufs = ctx.saved_tensors
        fold = lambda x: x[0] if x.dim() == 4 else x  # noqa: E731
        q3, bufs3 = fold(q), [fold(b) for b in bufs]
        g3 = fold(d_out.contiguous())
        acc = [torch.zeros(q3.shape, dtype=torch.float32, device=q.device) for _ in range(3)]
        dscores = ops.mix_experts_bwd(bufs3, g3)
        sc = routing_score[0].to(q.dtype).contiguous()  # what ops.mix_experts read in the forward

        def weight_of(_, o):  # the launch wrote expert e's buffer: its output enters the mixture with scores[:, e]
            e = next(i for i, b in enumerate(bufs3) if b.data_ptr() == o.data_ptr())
            return sc[:, e]

        launches = _bind_launches(ctx.launches, q3, fold(k), fold(v), bufs3)
        _replay_backward(launches, g3, acc[0], acc[1], acc[2], weight_of, ctx.algorithm)
        grads = [torch.empty_like(q3) for _ in range(3)]
        ops.cast_grads(acc, grads)
        d_sc = torch.zeros_like(routing_score)  # batch items > 0 are not read by the forward
        d_sc[0] = dscores.to(routing_score.dtype)
        dq, dk, dv = (g.view(q.shape) for g in grads)
        return dq, dk, dv, d_sc, None, None, None, None, None, None, None


def soft_mixture_attention_autograd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routing_score: torch.Tensor,
                                    geom: RoutedGeometry, *, model: str, text_len: int = 0, text_valid: int = 0,
                                    scale: Optional[float] = None, backward: Optional[str] = None,
                                    fidelity: Optional[list] = None) -> torch.Tensor:
    """`soft_mixture_attention` as a differentiable operator (router training: the loss reaches the routing scores and,
    through q, k, v, every earlier layer).  The forward is the same launches and gives the same bits; it keeps q, k, v, the
    scores, the three expert outputs and the launches as recorded.  The backward zeroes three float32 (H,N,D) buffers,
    takes dscores[h][e] = <d_out[h], x_e[h]> (ops.mix_experts_bwd), replays every forward launch through ops.attn_bwd with
    the weight scores[:, e] of its expert, and rounds dq, dk, dv once (ops.cast_grads).  The coreset keep / drop lists and
    the sliding-tile tables are constants of the backward (the reference ranks with argsort: no gradient flows through the
    selection there either, coreset_select.py:98-124).  dk / dv are not bit-reproducible (float atomics); dq and dscores are.
    `backward`: "query_major" (the above) or "key_major" (per launch ops.attn_bwd_stats, then ops.attn_bwd_key_major: dq is
    a sum of float atomics too) or "deterministic" (per launch ops.attn_bwd_stats, ops.attn_bwd_dq, ops.attn_bwd_dkv: no
    atomics -- dq, dk, dv and dscores are all bit-reproducible, the launches meeting in the shared buffers in stream order);
    None follows `set_attention_backward` / VORTA_ATTENTION_BACKWARD, read when the forward runs.  The forward is the same
    whichever it is.  q, k, v: contiguous (1,H,N,D), like the forward's.
    `fidelity`: as for `soft_mixture_attention` -- a list that receives one `ops.ExpertFidelity` (no gradient flows through it;
    a forward recomputed under gradient checkpointing appends again)."""
    return _SoftMixture.apply(q, k, v, routing_score, geom, model, text_len, text_valid, scale, backward, fidelity)


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, kv_valid, q_valid, scale, backward):
        ctx.algorithm = attention_backward(backward)
        out = torch.empty_like(q)
        Sq, Skv = q.shape[-2], k.shape[-2]
        launch = dict(n_q=Sq, n_kv=Skv if kv_valid is None else kv_valid, q_valid=Sq if q_valid is None else q_valid,
                      scale=scale)
        ops.attn_fwd(ops.fold_heads(q), ops.fold_heads(k), ops.fold_heads(v), ops.fold_heads(out), **launch)
        ctx.save_for_backward(q, k, v, out)
        ctx.launch = launch
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, out = ctx.saved_tensors
        f = ops.fold_heads
        acc = [torch.zeros(f(x).shape, dtype=torch.float32, device=q.device) for x in (q, k, v)]
        _attn_bwd_by(ctx.algorithm, f(q), f(k), f(v), f(out), f(d_out.contiguous()), acc[0], acc[1], acc[2], **ctx.launch)
        grads = [torch.empty_like(x) for x in (q, k, v)]
        ops.cast_grads(acc[:1], [f(grads[0])])
        ops.cast_grads(acc[1:], [f(grads[1]), f(grads[2])])
        return grads[0], grads[1], grads[2], None, None, None, None


def dense_attention_autograd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, kv_valid: Optional[int] = None,
                             q_valid: Optional[int] = None, scale: Optional[float] = None,
                             backward: Optional[str] = None) -> torch.Tensor:
    """`dense_attention` (the teacher path, use_original_attn=True: hunyuan.py:167-176, wan.py:134-145) as a differentiable
    operator: the same launch forward, ops.attn_bwd + ops.cast_grads backward.  (B,H,Sq,D) x (B,H,Skv,D), contiguous.
    `backward`: "query_major", "key_major" or "deterministic" (bit-reproducible dq, dk, dv), as for
    `soft_mixture_attention_autograd`."""
    return _Dense.apply(q, k, v, kv_valid, q_valid, scale, backward)


def _norm_rope_forward(x: torch.Tensor, weight, eps: float, cos, sin, rope_tokens, across_heads: bool) -> torch.Tensor:
    """out of place: a fresh contiguous (.., H, N, D) copy of x, normalised and rotated by the in-place kernel"""
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
        raise ValueError("qk_norm_rope_autograd takes a (H,N,D) or (1,H,N,D) view")
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device).copy_(x)
    ops.qk_norm_rope(y[0] if y.dim() == 4 else y, weight, eps, cos=cos, sin=sin, rope_tokens=rope_tokens,
                     across_heads=across_heads)
    return y


def _norm_rope_backward(x: torch.Tensor, g: torch.Tensor, weight, eps: float, cos, sin, rope_tokens, across_heads: bool,
                        want_dweight: bool):
    """(dx, dweight float32 | None) of `_norm_rope_forward`; dx in x's own layout (a transposed projection view stays one)"""
    fold = lambda t: t[0] if t.dim() == 4 else t  # noqa: E731
    if g.stride(-1) != 1 or any(st % 8 for st in g.stride()[:-1]) or g.data_ptr() % 16:
        g = g.contiguous()
    dx = torch.empty_like(x)
    _, dw = ops.qk_norm_rope_bwd(fold(x), fold(g), weight, eps, cos=cos, sin=sin, rope_tokens=rope_tokens,
                                 across_heads=across_heads, want_dweight=want_dweight, dx=fold(dx))
    return dx, dw


class _QkNormRope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps, cos, sin, rope_tokens, across_heads):
        y = _norm_rope_forward(x, weight, eps, cos, sin, rope_tokens, across_heads)
        ctx.save_for_backward(x, weight, cos, sin)
        ctx.rest = (eps, rope_tokens, across_heads)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, cos, sin = ctx.saved_tensors
        eps, rope_tokens, across_heads = ctx.rest
        dx, dw = _norm_rope_backward(x, g, weight, eps, cos, sin, rope_tokens, across_heads,
                                     weight is not None and ctx.needs_input_grad[1])
        if dw is not None:
            dw = dw.to(weight.dtype).view(weight.shape)
        return dx, dw, None, None, None, None, None


def qk_norm_rope_autograd(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float, cos: Optional[torch.Tensor] = None,
                          sin: Optional[torch.Tensor] = None, rope_tokens: Optional[int] = None,
                          across_heads: bool = False) -> torch.Tensor:
    """`ops.qk_norm_rope` (RMSNorm + rotary embedding of q or k, hunyuan.py:62-104 / wan.py:85-100) as a differentiable,
    OUT-OF-PLACE operator.  The in-place kernel would overwrite the output of a `Linear` behind autograd's back, so the
    forward copies x into a fresh contiguous (H,N,D) buffer, runs the kernel on the copy (the same bits as the in-place op
    on a copy) and keeps x, the weight and the tables; the backward is one `ops.qk_norm_rope_bwd` pass.  That extra copy
    of q and of k is the price of training.  x: a (H,N,D) or (1,H,N,D) view with contiguous rows, e.g. the transposed view
    of a (1,N,H*D) projection; gradients for x (in x's layout) and weight only -- cos / sin are constants.
    rope_tokens None: every token the tables cover."""
    return _QkNormRope.apply(x, weight, eps, cos, sin, rope_tokens, across_heads)


def dense_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, kv_valid: Optional[int] = None,
                    q_valid: Optional[int] = None, out: Optional[torch.Tensor] = None,
                    scale: Optional[float] = None) -> torch.Tensor:
    """The --native_attention path: every head dense (hunyuan.py:167-176, wan.py:134-145).  (B,H,Sq,D) x (B,H,Skv,D)."""
    if out is None:
        out = torch.empty_like(q)
    Sq, Skv = q.shape[-2], k.shape[-2]
    from . import torch_ops  # noqa: F401  (the launch goes through the custom op: traceable, same launcher)
    torch.ops.vorta.attn_fwd(ops.fold_heads(q), ops.fold_heads(k), ops.fold_heads(v), ops.fold_heads(out), Sq,
                             Skv if kv_valid is None else kv_valid, q_valid=Sq if q_valid is None else q_valid,
                             scale=0.0 if scale is None else scale)
    return out


_GEOMETRY_CACHE: Dict[tuple, RoutedGeometry] = {}
_GEOMETRY_CACHE_MAX = 48


def geometry_for(latent, tile, window, group, rate, device, row_map: Optional[torch.Tensor] = None,
                 partial: Optional[bool] = None) -> RoutedGeometry:
    """Process-wide cache: the tables are built once per geometry, not once per layer call.
    `partial`: as RoutedGeometry's (None = the process-wide switch, read here)."""
    partial = partial_geometry() if partial is None else bool(partial)
    key = (tuple(latent), tuple(tile), tuple(window), tuple(group), float(rate), str(device),
           None if row_map is None else (row_map.data_ptr(), row_map.numel()), partial)
    g = _GEOMETRY_CACHE.pop(key, None)
    if g is None:
        g = RoutedGeometry(latent, tile, window, group, rate, torch.device(device), row_map=row_map, partial=partial)
        # bounded: a geometry holds its sliding-tile tables (13 MB at Hunyuan-129f) and, under sequence parallelism, there is one
        # per distinct slot count of a rank (slot groups and uneven placements: up to ~2 H / P of them per resolution); the least
        # recently used one goes when a process has seen more than this many (the row maps they are keyed on are never freed)
        while len(_GEOMETRY_CACHE) >= _GEOMETRY_CACHE_MAX:
            _GEOMETRY_CACHE.pop(next(iter(_GEOMETRY_CACHE)))
    _GEOMETRY_CACHE[key] = g  # most recently used last
    return g


def sp_soft_mixture_attention(q, k, v, T, routing_score, **kw) -> torch.Tensor:
    """`soft_mixture_attention` under sequence parallelism, forward only: attention/_sp.py (imported on use: it builds on
    this module)"""
    from .attention._sp import sp_soft_mixture_attention as fn
    return fn(q, k, v, T, routing_score, **kw)


def sp_soft_mixture_attention_autograd(q, k, v, T, routing_score, **kw) -> torch.Tensor:
    """`soft_mixture_attention_autograd` under sequence parallelism (differentiable exchange): attention/_sp.py; `backward=`
    as there (None: `set_attention_backward` / VORTA_ATTENTION_BACKWARD, read when the forward runs)"""
    from .attention._sp import sp_soft_mixture_attention_autograd as fn
    return fn(q, k, v, T, routing_score, **kw)
