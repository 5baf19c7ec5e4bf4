"""Self-test of the footprint harness (tests/footprint.py) — no GPU: every case builder of tests/test_footprint_gpu.py runs through the
interpreter on host arenas.  That proves the arena arithmetic (pointers, strides, guard geometry) and the reference itself before a
kernel ever sees them: the interpreter leaves every guard intact, reads no NaN, and the padded case's payload equals the dense case's;
vmv_gemm_served_tile answers what the two literal exception tables claim; and a stray element is reported with its coordinates."""
import ctypes as C

import pytest
import torch

from videomv_amd import _lib as L
from tests import footprint as FP
from tests.test_footprint_gpu import FALLBACKS, REJECTS, gemm_expectation, test_every_live_tile_is_in_the_matrix as _live_tiles


def host_check(case, twin=None):
    for k, a in case.arenas.items():
        assert a.holds(0, a.rows * a.ld), (case.name, k)          # the interpreter's [rows][ld] view from the kernel's pointer ends inside the arena
        assert a.ptr(a.buf) % (16 if a.col_off % 8 == 0 else 8) == 0, (case.name, k)
    ref = case.run_ref()
    rep = case.guards_report(ref)
    assert not rep, rep
    for name in case.outs:
        assert torch.isfinite(ref.payload(name).float()).all(), f"{case.name}.{name}: the reference read a poisoned element"
    assert not case.inputs_report(ref), case.inputs_report(ref)       # inputs are not written
    if twin is not None:
        d = twin.run_ref()
        for name in case.outs:
            assert torch.equal(ref.payload(name), d.payload(name)), f"{case.name}.{name}: padded and dense references differ"
    return ref


def test_every_live_tile_is_in_the_matrix():
    _live_tiles()


@pytest.mark.parametrize("layout", FP.LAYOUTS)
def test_gemm_cases_on_the_host(layout):
    ran = 0
    for tname in FP.GENERIC:
        case = FP.gemm_case(tname, layout)
        if gemm_expectation(case, tname, layout):          # (asserts the error code / the serving tile of the two tables)
            host_check(case, FP.gemm_case(tname, layout, dense=True))
            ran += 1
    assert ran == len(FP.GENERIC) - len(REJECTS.get(layout, {}))


def test_exception_tables_are_minimal():
    """an entry of either table that the library no longer needs is stale: the combination must then run on its own kernel"""
    lib = L.load()
    for layout, tab in REJECTS.items():
        for tname, code in tab.items():
            assert code < 0 and tname not in FALLBACKS.get(layout, {})
    for layout, tab in FALLBACKS.items():
        for tname, want in tab.items():
            assert want != tname and want in FP.TILES
            p = (lambda c: c.build(c.on("cpu")))(FP.gemm_case(tname, layout))
            assert lib.vmv_gemm_served_tile(C.byref(p)) != FP.tile_id(tname)


@pytest.mark.parametrize("key", list(FP.SPECIAL))
def test_special_gemm_cases_on_the_host(key):
    lib = L.load()
    case = FP.SPECIAL[key](key)
    p = case.build(case.on("cpu"))
    assert lib.vmv_gemm_validate(C.byref(p)) == 0 and lib.vmv_gemm_served_tile(C.byref(p)) == case.tile
    host_check(case, FP.SPECIAL[key](key, dense=True))


def test_row_attention_and_glue_cases_on_the_host():
    host_check(FP.ff_case(M=40), FP.ff_case(M=40, dense=True))
    assert L.load().vmv_ff_fused_ok(C.byref((lambda c: c.build(c.on("cpu")))(FP.ff_case()))) == 1
    for kind, rows, n in (("normal", 5, 68), ("normal", 258, 4), ("huge", 5, 1000), ("dominant", 1, 4096)):
        ref = host_check(FP.softmax_case(rows, n, kind), FP.softmax_case(rows, n, kind, dense=True))
        assert float((ref.payload("p").double().sum(dim=1) - 1).abs().max()) <= 2.0 ** -8 + n * 2.0 ** -25
    for stats in (False, True):
        host_check(FP.layernorm_case(37, 320, stats), FP.layernorm_case(37, 320, stats, dense=True))
    for form in ("apply", "fused", "table"):
        host_check(FP.groupnorm_case(form), FP.groupnorm_case(form, dense=True))
    for key in FP.ATTN_CASES:
        host_check(FP.attention_case(key), FP.attention_case(key, dense=True))
    for name in FP.GLUE:
        host_check(FP.GLUE[name]())


def test_a_stray_store_is_reported_with_its_coordinates():
    """one element written by the test itself outside the payload — past column N of a tail-tile row, in the row after the last tile,
    in the left pad — is found and named: arena row / column and the tile row / column they fall in"""
    case = FP.gemm_case("256x128", "a")               # M = 257, N = 136: payload rows [8, 265) x columns [8, 144) of 144-wide rows
    a = case.arenas["out"]
    assert (a.rows, a.width, a.ld, a.col_off, a.gb, a.ga, a.tile) == (257, 136, 144, 8, 8, 512, (256, 128))
    b = case.run_ref()
    assert case.guards_report(b) == ""
    rows = b.buf("out").view(-1, a.ld)
    rows[a.gb + 257, a.col_off + 130] = 1.0          # the row below the 1-row tail tile, a column of the 8-column tail tile
    assert a.stray(b.buf("out")) == [(265, 138, 1, 1)]
    rep = case.guards_report(b)
    assert "arena (row 265, col 138) = tile (row 1, col 1)" in rep and "gemm[256x128-a].out" in rep
    rows[a.gb + 3, 2] = 0.0                          # the left pad of payload row 3
    rows[2, 9] = 0.0                                 # a guard row before the payload
    assert a.stray(b.buf("out")) == [(2, 9, -1, 0), (11, 2, 0, -1), (265, 138, 1, 1)]
    # a mis-sized helper call: the launch believes the rows are 8 elements narrower than the arena — its row 1 starts in row 0's tail
    small = FP.Arena(4, 8, "f32", ld=16, col_off=4, g_before=2, g_after=2)
    wrong = small.buf[:120].view(-1, 12)                   # [rows][ld = 12] view of a 16-wide arena
    wrong[3, 4:8] = 0.5                              # "payload row 1, columns 0..3" at ld 12 = arena elements 40..43 = (row 2, cols 8..11): inside
    assert small.stray(small.buf) == []
    wrong[4, 4:6] = 0.5                              # elements 52, 53 = arena (row 3, cols 4, 5): payload again
    wrong[5, 4:6] = 0.5                              # elements 64, 65 = arena (row 4, cols 0, 1): the left pad
    assert small.stray(small.buf) == [(4, 0, 2, -4), (4, 1, 2, -3)]
    # the 16-bit pattern is checked bit for bit: the same VALUE in another encoding (-0.0 vs 0.0 style) cannot hide a store
    e = FP.Arena(2, 8, "elem", ld=16, col_off=8)
    e.buf.view(torch.int16)[3] = FP.PAT16 ^ 1
    assert e.stray(e.buf) == [(0, 3, -8, -5)]
