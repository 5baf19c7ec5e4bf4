"""`not gpu`: the policy and the ABI of the row-stationary temporal convolution (csrc/gemm_trs.hip, VMV_TILE_TRS = 32; include/vmv.h
vmv_gemm_trs_ok) — host logic only, no launch — and the engine's use of it."""
import ctypes as C

import torch

from videomv_amd import _lib as L
from videomv_amd import ops
from tests import plan_interp

X = 1 << 20        # any 16-byte aligned non-null address: nothing is dereferenced


def tconv(B, F_, Pp, Cc=320, N=320, fold=True, tile=L.TILE_AUTO, **kw):
    if fold:
        kw.update(gn_table=X, gn_rows_per_stat=F_ * Pp, gn_silu=True)
    return ops.gemm_params(B * F_ * Pp, N, ops.temporal_segs(X, Cc, Cc), X, X, N, bias=X, geom=ops.Geom(F=F_, P=Pp), tile=tile, **kw)


def test_trs_policy():
    lib = L.load()
    ok = lambda p: lib.vmv_gemm_trs_ok(C.byref(p))
    served = lambda p: lib.vmv_gemm_served_tile(C.byref(p))
    assert L.TRS_TILE == 32 and lib.vmv_abi_version() == 12
    # the bench's folded first-level temporal convolution: both CFG branches, and the shared prefix (one branch); with the block's residual
    for B in (2, 1):
        for kw in ({}, dict(residual=X, ldr=320)):
            p = tconv(B, 24, 40 * 64, **kw)
            assert ok(p) == 1 and served(p) == L.TRS_TILE and lib.vmv_gemm_pick_tile(C.byref(p)) == L.TRS_TILE
    # not served: C = 640, F = 20, the plain form, item counts under the threshold (128 items = 26 row tiles of 16 pixels x 5 groups)
    assert ok(tconv(2, 24, 40 * 64 // 4, Cc=640, N=640)) == 0
    assert ok(tconv(2, 20, 40 * 64)) == 0
    plain = tconv(2, 24, 40 * 64, fold=False)
    assert ok(plain) == 0 and served(plain) == L.TILE_X256x320
    assert ok(tconv(1, 24, 16 * 25)) == 0 and served(tconv(1, 24, 16 * 25)) == L.TILE_TFR         # 25 x 5 = 125 items
    assert ok(tconv(1, 24, 16 * 26)) == 1 and served(tconv(1, 24, 16 * 26)) == L.TRS_TILE         # 26 x 5 = 130 items
    # more samples than norm tables fit in LDS: the folded form stays where it was
    assert ok(tconv(9, 24, 16 * 26)) == 0
    # 24 x 32 x 32: the frame-resident kernel keeps the shapes its own policy takes, plain and folded
    assert served(tconv(2, 24, 1024, fold=False)) == L.TILE_TFR
    assert ok(tconv(2, 24, 1024)) == 0 and served(tconv(2, 24, 1024)) == L.TILE_TFR
    # a forced tile also runs the unfolded form and small shapes; it refuses what the kernel does not serve
    assert served(tconv(1, 12, 5, fold=False, tile=L.TRS_TILE)) == L.TRS_TILE
    assert served(tconv(1, 16, 5, N=96, tile=L.TRS_TILE)) == L.TRS_TILE
    assert lib.vmv_gemm_validate(C.byref(tconv(1, 20, 5, tile=L.TRS_TILE))) == -1
    assert lib.vmv_gemm_validate(C.byref(tconv(1, 24, 5, Cc=640, N=640, tile=L.TRS_TILE))) == -1
    assert lib.vmv_gemm_validate(C.byref(tconv(1, 24, 5, N=48, tile=L.TRS_TILE))) == -1
    bad = tconv(2, 24, 5, tile=L.TRS_TILE); bad.gn_rows_per_stat = 24 * 5 * 2
    assert lib.vmv_gemm_validate(C.byref(bad)) == -1
    bad = tconv(1, 24, 5, fold=False, tile=L.TRS_TILE); bad.gn_silu = 1
    assert lib.vmv_gemm_validate(C.byref(bad)) == -1
    # the capped-grid entry point is for the forced tile only
    assert lib.vmv_gemm_trs_blocks(C.byref(tconv(1, 24, 5)), 2, None) == -1
    assert lib.vmv_gemm_trs_blocks(C.byref(tconv(1, 24, 5, tile=L.TRS_TILE)), 0, None) == -1


def test_trs_threshold_env(monkeypatch):
    lib = L.load()
    p = tconv(2, 24, 9)
    assert lib.vmv_gemm_trs_ok(C.byref(p)) == 0
    monkeypatch.setenv("VMV_TRS_MIN_ITEMS", "1")
    assert lib.vmv_gemm_trs_ok(C.byref(p)) == 1 and lib.vmv_gemm_served_tile(C.byref(p)) == L.TRS_TILE


def _engine(monkeypatch, H, W):
    plan_interp.install(monkeypatch)
    from videomv_amd.unet_engine import UNetEngine, param_shapes
    cfg = dict(in_dim=4, dim=320, context_dim=1024, out_dim=4, dim_mult=[1, 2], num_heads=8, head_dim=64, num_res_blocks=1,
               attn_scales=[1.0, 0.5], camera_dim=16, use_camera_condition=True, use_fps_condition=False)
    sd = {k: torch.zeros(s) for k, s in param_shapes(cfg).items()}
    return UNetEngine(cfg, sd, 2, 24, H, W, 77, torch.device("cpu"), n_t=1)


def test_engine_keeps_small_plans_and_folds_large_ones(monkeypatch):
    """A small latent (24 x 8 x 8: 8 row tiles x 5 groups = 40 items) records the op list it recorded before the kernel existed — the
    same as with the kernel switched off by an unreachable threshold; with the threshold lowered the first level's temporal
    convolutions are recorded as statistics + table + folded GEMM and the apply launches are gone."""
    monkeypatch.setenv("VMV_TRS_MIN_ITEMS", str(1 << 40))
    off = _engine(monkeypatch, 8, 8).S.labels
    monkeypatch.delenv("VMV_TRS_MIN_ITEMS")
    eng = _engine(monkeypatch, 8, 8)
    assert list(eng.S.labels) == list(off)
    fold0 = [p for op, p in eng.S.recorded if op == L.OP_GEMM and p.gn_table and p.nseg == 3]
    monkeypatch.setenv("VMV_TRS_MIN_ITEMS", "1")
    on = _engine(monkeypatch, 8, 8)
    folded = [p for op, p in on.S.recorded if op == L.OP_GEMM and p.gn_table and p.nseg == 3 and p.seg[0].k == 320]
    assert len(folded) > len(fold0) and len(folded) % 4 == 0 and all(on.S.lib.vmv_gemm_trs_ok(C.byref(p)) == 1 for p in folded)
    # every folded convolution traded its norm's apply (at this size: the one-launch statistics + apply form) for a table launch
    count = lambda e, *ops_: sum(1 for op, _ in e.S.recorded if op in ops_)
    n = len(folded) - len(fold0)
    assert count(eng, L.OP_GN_APPLY, L.OP_GN_FUSED) - count(on, L.OP_GN_APPLY, L.OP_GN_FUSED) == n
    assert count(on, L.OP_GN_TABLE) - count(eng, L.OP_GN_TABLE) == n
