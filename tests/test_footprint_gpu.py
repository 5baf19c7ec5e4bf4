"""The store footprint and the strided operands of every kernel — `pytest -m gpu` (harness: tests/footprint.py).

Every launch runs on arenas: the output between guard rows and guard columns that must keep their bit pattern (no tolerance), the inputs
between NaN, so that no kernel writes outside [M][N_out] of a strided output and none reads outside [rows][k] of a strided source.  The
payload is checked against the interpreter run on a host copy of the same arenas at the tolerance tests/test_kernels_gpu.py states for
the dense test of the same op (its `check`, per-op tol_l2 / tol_max, the TS factor); where the padded launch takes the dense launch's
store path it must also equal the dense launch bit for bit (accumulation order depends on the tile map, not on the strides).

A test id that names a tile proves nothing about the kernel that produced the numbers — forced tiles fall back when their launcher declines
— so every GEMM case asserts vmv_gemm_served_tile(p) == the forced tile, and the ONLY exceptions are the two literal tables below.
"""
import ctypes as C

import pytest
import torch

from videomv_amd import _lib as L
from tests import footprint as FP
from tests.test_kernels_gpu import TS, check

pytestmark = pytest.mark.gpu

EINVAL = -1
# (layout -> tile -> VMV_E* code) combinations a launcher rejects by contract: vmv_gemm_validate must answer exactly this code
REJECTS = {
    # the wide tile has the staged 16-byte epilogue only (16-bit output, ldo % 8 == 0) unless split-K hands the stores to the reduce pass
    "b": {"X256x320": EINVAL, "X256x256": EINVAL, "X256x128": EINVAL, "X512x128": EINVAL},
    "c": {"X256x320": EINVAL, "X256x256": EINVAL, "X256x128": EINVAL, "X512x128": EINVAL},
    # GEGLU pairs 16-column blocks: no 160-column tile; of the wide tiles only the 256 x 256 form carries the fused epilogues
    "f": {"128x160": EINVAL, "256x160": EINVAL, "G128x160": EINVAL, "P256x160": EINVAL, "PP256x160": EINVAL, "Q96x160": EINVAL,
          "X256x320": EINVAL, "X256x128": EINVAL, "X512x128": EINVAL},
    # the 8 x 1 wave grid has no split-K form
    "h": {"X512x128": EINVAL},
    # grouped weights: the generic kernel and the 128-column LDS-DMA kernels (vmv.h)
    "i": {"128x160": EINVAL, "256x160": EINVAL, "G128x160": EINVAL, "P256x160": EINVAL, "PP256x128": EINVAL, "PP256x160": EINVAL,
          "Q128x128": EINVAL, "Q96x160": EINVAL, "X256x320": EINVAL, "X256x256": EINVAL, "X256x128": EINVAL, "X512x128": EINVAL},
    # the phased up-convolution lives in the three 256-row wide tiles only
    "j": {"128x128": EINVAL, "128x160": EINVAL, "128x64": EINVAL, "64x64": EINVAL, "256x128": EINVAL, "256x160": EINVAL, "G128x128": EINVAL,
          "G128x160": EINVAL, "P256x128": EINVAL, "P256x160": EINVAL, "PP256x128": EINVAL, "PP256x160": EINVAL, "Q128x128": EINVAL,
          "Q96x160": EINVAL, "X512x128": EINVAL},
    # in-loop LayerNorm statistics: the one-block-per-CU persistent kernels (and the row-stationary kernel, below)
    "k_inline": {"128x128": EINVAL, "128x160": EINVAL, "128x64": EINVAL, "64x64": EINVAL, "256x128": EINVAL, "256x160": EINVAL,
                 "G128x128": EINVAL, "G128x160": EINVAL, "PP256x128": EINVAL, "PP256x160": EINVAL, "Q128x128": EINVAL, "Q96x160": EINVAL,
                 "X256x320": EINVAL, "X256x256": EINVAL, "X256x128": EINVAL, "X512x128": EINVAL},
}
# (layout -> tile -> serving tile) combinations that fall back: the case runs, on the kernel named here
_GATHER = {"P256x128": "256x128", "P256x160": "256x160", "Q128x128": "256x128", "Q96x160": "256x160"}      # persistent kernels: linear segments, no split-K
FALLBACKS = {
    "g_s1": dict(_GATHER), "g_s2": dict(_GATHER), "g_ups": dict(_GATHER), "g_t": dict(_GATHER), "h": dict(_GATHER),
    # a folded LayerNorm (rowstat) lives in the persistent kernels, the generic kernel and the 256 x 256 wide tile: every other forced
    # tile is re-routed to the 128-column persistent kernel (N = BN + 8 is no multiple of 160)
    "k_rowstat": {"256x128": "P256x128", "256x160": "P256x128", "G128x128": "P256x128", "G128x160": "P256x128", "PP256x128": "P256x128",
                  "PP256x160": "P256x128", "X256x320": "P256x128", "X256x128": "P256x128", "X512x128": "P256x128"},
}


def compare(case, got, ref):
    for name, tol in case.outs.items():
        a, b = got.payload(name), ref.payload(name)
        if tol == "exact":
            assert torch.equal(a.cpu(), b), f"{case.name}.{name}"
        elif tol == "stats":
            assert torch.allclose(a.cpu(), b, rtol=2e-5, atol=2e-6), f"{case.name}.{name}"       # (as test_layernorm_stats_out)
        else:
            check(a, b, **tol)


def run_case(case, twin=None):
    """reference on the host arenas, the kernel on device arenas: guards bit-identical, payload within the op's tolerance, and — `twin`
    = the same launch on dense buffers — bit-identical to the dense launch"""
    ref = case.run_ref()
    assert not case.guards_report(ref), "the reference itself strays: " + case.guards_report(ref)
    got = case.run_gpu()
    rep = case.guards_report(got)
    assert not rep, rep
    assert not case.inputs_report(got), case.inputs_report(got)
    compare(case, got, ref)
    if twin is not None:
        d = twin.run_gpu()
        for name in case.outs:
            assert torch.equal(got.payload(name), d.payload(name)), f"{case.name}.{name}: the padded payload differs from the dense launch's"
    return got, ref


def gemm_expectation(case, tname, layout):
    """the served-tile contract of a GEMM case: returns False when the launch is rejected by contract (asserted), True when it runs"""
    lib = L.load()
    p = case.build(case.on("cpu"))
    code = REJECTS.get(layout, {}).get(tname)
    if code is not None:
        assert lib.vmv_gemm_validate(C.byref(p)) == code and lib.vmv_gemm_served_tile(C.byref(p)) == code, (tname, layout)
        return False
    assert lib.vmv_gemm_validate(C.byref(p)) == 0, (tname, layout)
    want = FALLBACKS.get(layout, {}).get(tname, tname)
    assert lib.vmv_gemm_served_tile(C.byref(p)) == FP.tile_id(want), (tname, layout, want)
    return True


def test_every_live_tile_is_in_the_matrix():
    """The live VMV_TILE_* ids of _lib.py are exactly the harness's table plus the retired ids (which the library refuses), and every
    live id runs layout (a) on its own kernel: no exception-table entry covers it."""
    lib = L.load()
    ids = {n[5:]: getattr(L, n) for n in dir(L) if n.startswith("TILE_") and n != "TILE_AUTO"}
    assert set(ids) == set(FP.TILES) | set(FP.RETIRED), set(ids) ^ (set(FP.TILES) | set(FP.RETIRED))
    for t in FP.RETIRED:
        p = FP.gemm_case("128x128", "a").build(FP.gemm_case("128x128", "a").on("cpu"))
        p.tile = ids[t]
        assert lib.vmv_gemm_validate(C.byref(p)) == EINVAL
    for t in FP.GENERIC:
        assert t not in REJECTS.get("a", {}) and t not in FALLBACKS.get("a", {})
    for lay, tab in list(REJECTS.items()) + list(FALLBACKS.items()):
        assert lay in FP.LAYOUTS and set(tab) <= set(FP.GENERIC), lay
    served_special = {FP.RS_CASES[k][0] for k in FP.RS_CASES} | {"TFR", "TQA", "HALO"}
    assert set(FP.TILES) == set(FP.GENERIC) | served_special


@pytest.mark.parametrize("layout", FP.LAYOUTS)
@pytest.mark.parametrize("tname", FP.GENERIC)
def test_gemm_footprint(tname, layout):
    """The generic tiles x the layouts (a) padded rows + column offset (staged path), (b) ldo = N + 4 (8-byte path), (c) fp32 with
    ldo = N + 4, (d / d2) source slices, one and two sources of different ld, (e) residual slice + row vector from an offset base,
    (f) GEGLU with N_out padded, (g) spatial taps stride 1 / stride 2 / nearest-x2 and temporal taps with padded ld (zero-padded taps
    next to NaN rows), (h) split-K = 2 with the workspace in an arena, (i) grouped weights, (j) the phased x2 up-convolution (the row
    scatter hits exactly the 4 Mp payload rows), (k) folded LayerNorm, rowstat and in-loop forms.  Nothing is skipped: a combination
    either runs on the kernel it names (or the FALLBACKS entry) or is in REJECTS with the code the library must answer."""
    case = FP.gemm_case(tname, layout)
    if not gemm_expectation(case, tname, layout):
        return
    twin = FP.gemm_case(tname, layout, dense=True) if layout in FP.BITWISE else None
    if twin is not None:
        lib = L.load()
        assert lib.vmv_gemm_served_tile(C.byref(twin.build(twin.on("cpu")))) == lib.vmv_gemm_served_tile(C.byref(case.build(case.on("cpu"))))
    run_case(case, twin)


@pytest.mark.parametrize("key", list(FP.SPECIAL))
def test_gemm_footprint_special_kernels(key):
    """The kernels with their own shape contracts, each on its own tile id (served == forced, no exceptions): the row-stationary kernel
    (K = 320 / 640 / 512; 64 and 32 rows per wave; split and unsplit columns; source slice, residual, GEGLU, in-loop LayerNorm, folded
    GroupNorm), the frame-resident temporal convolution (ragged last block; residual; folded GroupNorm with and without SiLU), the fused
    q | k | v + temporal attention (pad columns, guard rows, column offset) and the halo convolution (images that are no multiple of the
    4 x 16 pixel tile, fp32 and 16-bit)."""
    lib = L.load()
    case = FP.SPECIAL[key](key)
    p = case.build(case.on("cpu"))
    assert lib.vmv_gemm_validate(C.byref(p)) == 0 and lib.vmv_gemm_served_tile(C.byref(p)) == case.tile
    run_case(case, FP.SPECIAL[key](key, dense=True))


@pytest.mark.parametrize("ln,res", [(True, True), (False, False)])
def test_ff_fused_footprint(ln, res):
    case = FP.ff_case(ln=ln, res=res)
    assert L.load().vmv_ff_fused_ok(C.byref(case.build(case.on("cpu")))) == 1
    run_case(case, FP.ff_case(ln=ln, res=res, dense=True))


# ------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("kind,rows,n", [("normal", r, n) for n in (4, 68, 1000, 4096) for r in (1, 5, 258)] + [("huge", 5, 1000), ("dominant", 258, 68),
                                                                                                                  ("dominant", 5, 4096)])
def test_softmax_rows_footprint(kind, rows, n):
    """vmv_softmax_rows against fp64 softmax(scale * s) of the fp32 scores: row counts that are no multiple of the 4 rows per block, row
    lengths from one vector to 16 per lane, lds = ldp = n + 4 from offset bases; every stored row sums to 1 within 2^-8 TS + n 2^-25 (the
    half-ulp of the 16-bit type on a unit sum, one subnormal rounding per element)."""
    case = FP.softmax_case(rows, n, kind)
    got, _ = run_case(case)
    sums = got.payload("p").double().sum(dim=1).cpu()
    bound = 2.0 ** -8 * TS + n * 2.0 ** -25
    print(f"softmax {kind} {rows} x {n}: max |row sum - 1| = {float((sums - 1).abs().max()):.3e} (bound {bound:.3e})")
    assert float((sums - 1).abs().max()) <= bound


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("rows,Cc", [(37, 320), (5, 512), (3, 2048), (66, 64)])
def test_layernorm_footprint(rows, Cc, stats):
    """vmv_layernorm with ldx = ldy = C + 8, row counts that leave the last block ragged at every lanes-per-row form; the stats_out form
    writes the guarded [rows][2] fp32 table and gets y = NULL"""
    run_case(FP.layernorm_case(rows, Cc, stats))


@pytest.mark.parametrize("form", ["apply", "fused", "table"])
def test_groupnorm_footprint(form):
    """two sources with ld = C0 + 8, ld1 = C1 + 8, ldy = C + 8; rows_per_stat = 50 with chunk_rows = 16; the partial workspace guarded"""
    run_case(FP.groupnorm_case(form))


@pytest.mark.parametrize("key", list(FP.ATTN_CASES))
def test_attention_footprint(key):
    """the output written through `om` into rows 64 wider than the heads, the head slices 32 columns in; q | k | v slices of padded rows;
    spatial, cross with kv_div, temporal, causal and head_dim 32 at the smallest shape the dense tests use"""
    run_case(FP.attention_case(key))


@pytest.mark.parametrize("name", list(FP.GLUE))
def test_glue_footprint(name):
    run_case(FP.GLUE[name]())
