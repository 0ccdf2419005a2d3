"""CPU-only checks of the per-head expert fidelity (include/vorta_hip.h vorta_expert_fidelity): exported symbols and the
structure size, argument validation before any launch (fake device addresses, never dereferenced on the host), the compiled
kernels' resources, the fake operator's shapes, and the host arithmetic on hand-made tables: `rel_error` / `psnr` edge rules,
`routes_from_fidelity`, `evaluate_routing`."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000  # a fake, 16-byte aligned device address


def _valid_args(heads=2, n_rows=8, mixed=True):
    from vorta_amd import _C
    a = _C.FidelityArgs()
    a.struct_size = ctypes.sizeof(_C.FidelityArgs)
    a.dtype, a.head_dim, a.heads, a.n_rows = _C.VORTA_BF16, 128, heads, n_rows
    for t in list(a.x) + ([a.mixed] if mixed else []):
        t.ptr, t.stride_h, t.stride_s = P, n_rows * 128, 128
    a.sq_ref, a.max_ref, a.sq_err, a.max_err, a.range_ref, a.ws = P, P + 64, P + 128, P + 256, P + 512, P + 1024
    return a


def test_symbols_abi_and_struct_size():
    from vorta_amd import _C
    lib = _C.lib()
    for name in ("vorta_expert_fidelity", "vorta_fidelity_args_size"):
        assert name in _C.SYMBOLS and getattr(lib, name) is not None
    assert lib.vorta_abi_version() == 9 == _C.ABI_VERSION  # a pure addition: the number stays
    assert lib.vorta_fidelity_args_size() == ctypes.sizeof(_C.FidelityArgs) == 24 + 4 * ctypes.sizeof(_C.Tensor) + 6 * 8
    assert lib.vorta_sizeof(16) == ctypes.sizeof(_C.NormRopeBwdArgs) and lib.vorta_sizeof(17) == -1  # 17 indices, as before
    from vorta_amd import build
    assert "expert_fidelity.hip" in build.SOURCES


def test_header_constants_match_the_binding():
    from vorta_amd import _C
    header = open(os.path.join(ROOT, "include", "vorta_hip.h")).read()
    assert int(re.search(r"#define VORTA_FIDELITY_PARTS (\d+)", header).group(1)) == _C.FIDELITY_PARTS
    assert int(re.search(r"#define VORTA_FIDELITY_WS_FLOATS (\d+)", header).group(1)) == _C.FIDELITY_WS_FLOATS
    macro = re.search(r"#define VORTA_FIDELITY_CHAIN\(n_rows\) (.*)", header).group(1)
    expr = macro.replace("(int64_t)", "").replace("VORTA_FIDELITY_PARTS", str(_C.FIDELITY_PARTS)).replace("/", "//")
    for n in (0, 1, 7, 64, 65, 1000, 1024, 1025, 119056, 75600, 1 << 24):
        assert eval(expr, {"n_rows": n}) == _C.fidelity_chain(n), n
    # the stated design point: Hunyuan-129f, 118 800 video + 256 text rows a head
    assert _C.fidelity_chain(119056) == 138 and 138 * 2.0 ** -24 < 1e-4
    assert "VORTA_FIDELITY_CHAIN" in open(os.path.join(ROOT, "vorta_amd", "csrc", "expert_fidelity.hip")).read()


def test_argument_validation_happens_before_any_launch():
    from vorta_amd import _C
    lib = _C.lib()
    call = lambda a: lib.vorta_expert_fidelity(ctypes.byref(a), None)  # noqa: E731
    EINVAL, EUNSUP, OK = _C.VORTA_EINVAL, _C.VORTA_EUNSUPPORTED, _C.VORTA_OK
    assert lib.vorta_expert_fidelity(None, None) == EINVAL
    a = _valid_args(heads=0)  # a valid block with no heads: OK, and nothing is launched
    assert call(a) == OK
    a = _valid_args(heads=0, mixed=False)
    assert call(a) == OK
    a = _valid_args()
    a.struct_size = 7
    assert call(a) == EINVAL
    for dt in (_C.VORTA_FP32, _C.VORTA_FP8E4M3, _C.VORTA_INT8):
        a = _valid_args()
        a.dtype = dt
        assert call(a) == EUNSUP
    a = _valid_args()
    a.head_dim = 64
    assert call(a) == EUNSUP
    for field in ("heads", "n_rows"):
        a = _valid_args()
        setattr(a, field, -1)
        assert call(a) == EINVAL
    for out in ("sq_ref", "max_ref", "sq_err", "max_err", "ws"):  # null outputs / workspace (also with no heads to write)
        for heads in (0, 2):
            a = _valid_args(heads=heads)
            setattr(a, out, None)
            assert call(a) == EINVAL, (out, heads)
    a = _valid_args()
    a.range_ref = None  # optional
    a.heads = 0
    assert call(a) == OK
    for out, off in (("sq_ref", 2), ("max_ref", 1), ("sq_err", 2), ("max_err", 3), ("range_ref", 2), ("ws", 4), ("ws", 8)):
        a = _valid_args()
        setattr(a, out, P + 2048 + off)
        assert call(a) == EINVAL, (out, off)
    for e in range(4):  # x[0..2] and mixed: null, pointer off 16 bytes, strides that break 16-byte rows
        for defect in ("null", "pointer", "stride_s", "stride_h"):
            a = _valid_args()
            t = a.x[e] if e < 3 else a.mixed
            if defect == "null":
                if e == 3:
                    continue  # a null `mixed` means "not given"
                t.ptr = None
            elif defect == "pointer":
                t.ptr = P + 8
            elif defect == "stride_s":
                t.stride_s = 132
            else:
                t.stride_h = 8 * 128 + 4
            assert call(a) == EINVAL, (e, defect)
    a = _valid_args(heads=0, n_rows=0)  # no rows to read: null expert outputs are accepted
    for t in a.x:
        t.ptr = None
    a.mixed.ptr = None
    assert call(a) == OK
    a = _valid_args(heads=(1 << 31) // 64)  # heads x parts must fit the grid
    assert call(a) == EINVAL


def test_missing_symbol_is_a_clear_error(tmp_path, monkeypatch):
    """`_C.py` refuses a library that lacks the entry point, naming it"""
    import shutil
    import subprocess
    from vorta_amd import _C
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("needs a C compiler")
    src = tmp_path / "old.c"
    src.write_text("\n".join(f"int {n}(void) {{ return 9; }}" for n in _C.SYMBOLS if n != "vorta_expert_fidelity") + "\n")
    so = tmp_path / "libold.so"
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    monkeypatch.setattr(_C, "LIB_PATH", str(so))
    monkeypatch.setattr(_C, "_lib", None)
    with pytest.raises(_C.VortaHipError, match="vorta_expert_fidelity"):
        _C.lib()


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")
def test_kernel_resources():
    """no scratch, no spill; four partial kernels (bf16 / fp16, with / without the mixed output) and the final one"""
    from vorta_amd import build
    res = build.kernel_resources("expert_fidelity.hip")
    assert len(res) == 5
    for name, r in res.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 64 and r["lds"] <= 256, (name, r)  # eight waves a SIMD fit in 64 registers


def test_python_surface_and_fake_shapes():
    import inspect
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vorta_amd import ops, routed, torch_ops  # noqa: F401
    from vorta_amd.attention import _sp, hunyuan, wan
    import vorta_amd.patch as patch
    assert ops.ExpertFidelity._fields[:4] == ("sq_ref", "max_ref", "sq_err", "max_err")
    for fn in (routed.soft_mixture_attention, routed.soft_mixture_attention_autograd, _sp.sp_soft_mixture_attention,
               _sp.sp_soft_mixture_attention_autograd, hunyuan.HunyuanVideoFlashAttnProcessorTripleTrain.__call__,
               wan.WanAttnProcessorTripleTrain.__call__):
        assert inspect.signature(fn).parameters["fidelity"].default is None, fn
    for name in ("expert_fidelity", "fidelity_of", "routes_from_fidelity", "evaluate_routing"):
        assert callable(getattr(patch, name))
    with pytest.raises(ops._C.VortaHipError):  # no CPU path
        ops.expert_fidelity([torch.zeros((1, 8, 128), dtype=torch.bfloat16)] * 3)
    assert "Tensor? mixed=None" in str(torch.ops.vorta.expert_fidelity.default._schema)
    with FakeTensorMode():
        x = torch.empty((3, 77, 128), dtype=torch.float16, device="cuda")
        for mixed in (None, x):
            out = torch.ops.vorta.expert_fidelity(x, x, x, mixed)
            assert [tuple(t.shape) for t in out] == [(3,), (3,), (3, 3), (3, 3), (3,)]
            assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in out)


def _fid(sq_ref, sq_err, max_ref=None, n=128, range_ref=None):
    from vorta_amd.ops import ExpertFidelity
    sq_ref, sq_err = torch.tensor(sq_ref, dtype=torch.float32), torch.tensor(sq_err, dtype=torch.float32)
    max_ref = sq_ref.sqrt() if max_ref is None else torch.tensor(max_ref, dtype=torch.float32)
    return ExpertFidelity(sq_ref, max_ref, sq_err, sq_err.sqrt(), None if range_ref is None else torch.tensor(range_ref), n)


def test_rel_error_edge_rules():
    inf, nan = float("inf"), float("nan")
    f = _fid([4.0, 0.0, 0.0, 1.0], [[1.0, 0.0, 16.0], [0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [nan, inf, 0.25]])
    rel = f.rel_error()
    assert rel.shape == (4, 3)
    assert rel[0].tolist() == [0.5, 0.0, 2.0]
    assert rel[1].tolist() == [0.0, inf, 0.0]   # sq_ref == 0: 0 where the error is 0, inf otherwise
    assert rel[2].tolist() == [0.0, 0.0, 0.0]
    assert math.isnan(rel[3, 0]) and rel[3, 1] == inf and rel[3, 2] == 0.5
    # a leading layer axis
    g = _fid([[4.0, 1.0]], [[[1.0, 1.0, 1.0], [0.0, 4.0, 1.0]]])
    assert g.rel_error().tolist() == [[[0.5, 0.5, 0.5], [0.0, 2.0, 1.0]]]


def test_psnr_conventions():
    """10 log10(peak^2 / mse): peak = max |x0| ("max_abs") or max x0 - min x0 ("range"), mse = sq_err / n"""
    f = _fid([100.0], [[2.0, 0.0, 8.0]], max_ref=[3.0], n=200, range_ref=[5.0])
    p = f.psnr()
    assert p[0, 0] == pytest.approx(10 * math.log10(9.0 / 0.01), abs=1e-4)
    assert p[0, 1] == float("inf")
    assert p[0, 2] == pytest.approx(10 * math.log10(9.0 / 0.04), abs=1e-4)
    assert f.psnr(over="range")[0, 0] == pytest.approx(10 * math.log10(25.0 / 0.01), abs=1e-4)
    with pytest.raises(ValueError):
        f.psnr(over="rms")
    with pytest.raises(ValueError):
        f._replace(n=0).psnr()
    with pytest.raises(ValueError):
        f._replace(range_ref=None).psnr(over="range")


GEOMETRY = dict(latent=(33, 45, 80), tile=(11, 9, 8), window=(3, 3, 3), group=(2, 3, 2), rate=0.5)


def test_expert_work_is_the_baseline_formula():
    from vorta_amd.patch import expert_work
    S, D, te = 33 * 45 * 80, 128, 40
    s_low, tok, n_kv = (S // 12) * 6, 11 * 9 * 8, 27
    full, low, sl = expert_work(GEOMETRY, te)
    assert full == 4.0 * (S + te) ** 2 * D and low == 4.0 * (s_low + te) ** 2 * D
    assert sl == 4.0 * D * (S * (n_kv * tok + te) + te * (S + te))
    full, low, sl = expert_work(GEOMETRY)
    assert round(low / full, 2) == 0.25 and round(sl / full, 2) == 0.18  # BASELINE.md's table, config 3
    # the other two spellings of a geometry, on the authors' 117-frame shape (the coreset window divides that latent)
    from vorta_amd.attention import get_group_info
    from vorta_amd.routed import RoutedGeometry
    g117 = dict(GEOMETRY, latent=(30, 45, 80), tile=(6, 9, 8))
    want = expert_work(g117, 7)
    assert round(want[1] / want[0], 2) == 0.25
    assert expert_work(RoutedGeometry(device=torch.device("cpu"), **g117), 7) == want
    kw = dict(latent_shape=g117["latent"], tile_size=g117["tile"], window_size=g117["window"],
              lowres_group_info=get_group_info(g117["latent"], g117["group"], g117["rate"]))
    assert expert_work(kw, 7) == want


def test_routes_from_fidelity_on_a_hand_made_table():
    from vorta_amd.patch import routes_from_fidelity
    # rel_error rows (coreset, sliding): both in, only coreset, only sliding, none, a tie, exact zeros, NaN
    f = _fid([[1.0] * 7], [[[0.0004, 0.0009, 9.0], [0.0004, 0.25, 9.0], [0.25, 0.0004, 9.0], [0.25, 0.25, 9.0],
                            [0.0025, 0.0025, 9.0], [0.0, 0.04, 9.0], [float("nan"), float("nan"), 9.0]]])
    table = routes_from_fidelity(f, 0.05)
    assert table.dtype == torch.int64 and table.shape == (1, 7)
    # cost order sliding < coreset < full: sliding wherever it is within the bound (a tie at the bound included)
    assert table.tolist() == [[2, 1, 2, 0, 2, 1, 0]]
    assert routes_from_fidelity(f, 0.05, geometry=GEOMETRY).tolist() == table.tolist()
    # a geometry whose sliding window covers every tile: the sliding expert costs what full attention costs, coreset is cheaper
    wide = dict(GEOMETRY, window=(3, 5, 10))
    assert routes_from_fidelity(f, 0.05, geometry=wide).tolist() == [[1, 1, 2, 0, 1, 1, 0]]
    # a bound of 0: full everywhere, unless an error is exactly 0
    assert routes_from_fidelity(f, 0.0).tolist() == [[0, 0, 0, 0, 0, 1, 0]]
    # the mixed column (9.0) is never a route
    assert routes_from_fidelity(f, 10.0).tolist() == [[2, 2, 2, 2, 2, 2, 0]]


def test_evaluate_routing_on_a_hand_made_table():
    from vorta_amd.patch import evaluate_routing, expert_work
    f = _fid([[1.0, 1.0, 1.0, 1.0], [4.0, 4.0, 4.0, 4.0]],
             [[[0.01, 0.04, 0.0]] * 4, [[1.0, 0.16, 0.0]] * 4])  # rel: layer 0 (0.1, 0.2), layer 1 (0.5, 0.2)
    experts = torch.tensor([[0, 1, 2, 2], [1, 1, 0, 2]])
    r = evaluate_routing(experts, f, GEOMETRY)
    assert r["experts"].tolist() == experts.tolist()
    assert r["worst_rel_error"].tolist() == pytest.approx([0.2, 0.5])
    assert r["mean_rel_error"].tolist() == pytest.approx([(0.0 + 0.1 + 0.2 + 0.2) / 4, (0.5 + 0.5 + 0.0 + 0.2) / 4])
    w = expert_work(GEOMETRY)
    assert r["flops_share"].tolist() == pytest.approx([(w[0] + w[1] + 2 * w[2]) / (4 * w[0]), (2 * w[1] + w[0] + w[2]) / (4 * w[0])])
    assert evaluate_routing(torch.zeros((2, 4), dtype=torch.int64), f, GEOMETRY)["flops_share"].tolist() == [1.0, 1.0]
    # scores: the first maximum; full attention where it is below tau_sparse; (L, B, H, 3) reads batch item 0
    scores = torch.tensor([[[0.2, 0.4, 0.4], [0.5, 0.5, 0.0], [0.1, 0.2, 0.7], [0.34, 0.33, 0.33]]] * 2)
    assert evaluate_routing(scores, f, GEOMETRY)["experts"].tolist() == [[1, 0, 2, 0]] * 2
    assert evaluate_routing(scores, f, GEOMETRY, tau_sparse=0.45)["experts"].tolist() == [[0, 0, 2, 0]] * 2
    batched = torch.stack([scores, scores.flip(-1)], dim=1)
    assert evaluate_routing(batched, f, GEOMETRY)["experts"].tolist() == [[1, 0, 2, 0]] * 2
    with pytest.raises(ValueError):
        evaluate_routing(experts[:1], f, GEOMETRY)
    with pytest.raises(ValueError):
        evaluate_routing(experts + 2, f, GEOMETRY)


def test_fidelity_of_refuses_without_a_measured_forward():
    from torch import nn
    from vorta_amd.patch import expert_fidelity, fidelity_of
    model = nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="expert_fidelity"):
        fidelity_of(model)
    with pytest.raises(ValueError, match="apply_vorta_transformer"):
        with expert_fidelity(model):
            pass
