"""Nearest-x2 + 3x3 convolution as four 2x2 phase convolutions (include/vmv.h: VmvGemmParams.phased), host side: the weight pre-sum, the
engine's choice between the phased and the nine-tap launch, the full-size plans and the argument validation.  No GPU."""
import ctypes
import dataclasses

import pytest
import torch
import torch.nn.functional as Fn

from oracle.unet_ref import UNetCfg, unet_forward
from oracle.weights import random_state_dict, unet_param_shapes
from tests import up4_ref
from tests.test_engine_cpu import CFG, _inputs, rel_l2


@pytest.mark.parametrize("n,Cc,N,IH,IW", [(3, 8, 12, 1, 1), (1, 8, 8, 2, 1), (2, 16, 8, 3, 5), (2, 8, 8, 5, 8)])
def test_phase_form_equals_upsampled_conv_fp64(n, Cc, N, IH, IW):
    """gather -> four matmuls with the summed weights -> scatter == conv2d(interpolate(nearest x2)) in fp64 (1 x 1 and 2 x 1 inputs: every
    tap at a border; odd sizes)."""
    from videomv_amd import packing as P
    g = torch.Generator().manual_seed(n * 100 + IH * 10 + IW)
    x = torch.randn(n, Cc, IH, IW, generator=g, dtype=torch.float64)
    w = torch.randn(N, Cc, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    ref = Fn.conv2d(Fn.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    W4 = P.up4_sum_weights(w)
    assert W4.shape == (4, N, 4 * Cc) and W4.dtype == torch.float64
    rows = up4_ref.up4_rows(x.permute(0, 2, 3, 1).reshape(n * IH * IW, Cc), n, IH, IW, W4, b)
    got = rows.view(n, 2 * IH, 2 * IW, N).permute(0, 3, 1, 2)
    assert float((got - ref).abs().max()) <= 1e-12


def test_packed_phase_weights_are_summed_in_fp32_and_rounded_once():
    """pack_conv3x3_up4: [4 N'][4 C'] phase-major, channels padded to 8 and rows to 4 as pack_conv3x3 does, elem(fp32 sum)."""
    from videomv_amd import _lib as L, packing as P
    w = torch.randn(6, 5, 3, 3, generator=torch.Generator().manual_seed(1))
    pk = P.pack_conv3x3_up4(w, torch.device("cpu"))
    assert pk.shape == (4 * 8, 4 * 8) and pk.dtype == L.elem()
    wp = torch.cat([w, torch.zeros(6, 3, 3, 3)], dim=1)
    W4 = P.up4_sum_weights(wp)
    for ph in range(4):
        assert torch.equal(pk[8 * ph:8 * ph + 6], W4[ph].to(L.elem())) and not pk[8 * ph + 6:8 * ph + 8].any()
    # phase (1, 1), tap (a, b) = (0, 0) of channel 2: kernel rows {0, 1} x columns {0, 1}
    assert torch.equal(pk[3 * 8 + 1, 2], w[1, 2, :2, :2].sum().to(L.elem()))


def _small_engine(taps=None):
    from videomv_amd.unet_engine import UNetEngine
    ocfg = UNetCfg(**{k: v for k, v in CFG.items() if k in {f.name for f in dataclasses.fields(UNetCfg)}})
    sd = random_state_dict(unet_param_shapes(ocfg), 99)
    B, F_, H, W, Lc = 2, 3, 8, 8, 5
    x, t, y, cam = _inputs(B, F_, H, W, Lc)
    eng = UNetEngine(CFG, sd, B, F_, H, W, Lc, torch.device("cpu"), n_t=B, taps=taps)
    eng.set_context(y)
    eng.set_camera(cam)
    eng.forward_rows(x, t)
    return eng, (sd, ocfg, x, t, y, cam)


def _phased(eng):
    from videomv_amd import _lib as L
    return [(lb, p) for lb, (op, p) in zip(eng.S.labels, eng.S.recorded) if op == L.OP_GEMM and p.phased]


def test_engine_records_and_executes_the_phased_launch(monkeypatch):
    """The 2 x 3 x 8 x 8 network of test_recorded_plan_matches_oracle with VMV_UP4_MIN_ROWS=1: the up convolution is ONE phased launch
    (96 rows per phase), the plan has as many ops as without the override and matches the oracle at that test's tolerances; without
    the override (the default minimum of rows per phase) nothing phased is recorded."""
    up4_ref.install(monkeypatch)
    monkeypatch.delenv("VMV_UP4_MIN_ROWS", raising=False)
    eng0, _ = _small_engine()
    assert not _phased(eng0)
    monkeypatch.setenv("VMV_UP4_MIN_ROWS", "1")
    taps = {}
    eng, (sd, ocfg, x, t, y, cam) = _small_engine(taps)
    ph = _phased(eng)
    n_up = sum(1 for blk in eng.outb for k, _, _ in blk if k == "up")
    assert len(ph) == n_up == 1 and eng.S.nops == eng0.S.nops
    p = ph[0][1]
    assert (p.M, p.N, p.ktot, p.nseg, p.ups, p.IH, p.IW, p.OH, p.OW) == (2 * 3 * 8 * 8, 128, 4 * 128, 4, 1, 4, 4, 8, 8)
    assert eng.S.lib.vmv_gemm_validate(ctypes.byref(p)) == 0
    taps_ref = {}
    eps_ref = unet_forward(sd, ocfg, x, t, y, cam, taps=taps_ref)
    for key, (act, h, w) in taps.items():
        mine = act.tensor().float().view(2 * 3, h, w, act.C).permute(0, 3, 1, 2)
        assert rel_l2(mine, taps_ref[key]) < 3e-2, key
    assert rel_l2(eng.eps_ncfhw(), eps_ref) < 2e-2
    d = rel_l2(eng.eps_ncfhw(), eng0.eps_ncfhw())
    assert 0 < d < 5e-3, d          # rounding-level, not bit-equal: the summed weights are rounded once


def test_full_size_plans_hold_the_phased_launches(monkeypatch):
    """The 24 x 40 x 64 and 24 x 32 x 32 plans (zero weights, recorded on the CPU): the Upsample convolutions are phased launches with
    K = 4 C that the library accepts, the launch count is unchanged, and their signatures carry the mode.  All three at 40 x 64; at
    32 x 32 the third-level one has 768 rows per phase — the size of the largest plan the host interpreter (nine-tap only) executes in
    tests/test_frame_parallel_cpu.py — and stays on nine taps under the default size rule (more than 768 rows per phase)."""
    from tests import plan_interp
    plan_interp.install(monkeypatch)
    monkeypatch.delenv("VMV_UP4_MIN_ROWS", raising=False)
    from videomv_amd import ops
    from videomv_amd.unet_engine import UNetEngine, param_shapes
    cfg = dict(in_dim=4, dim=320, context_dim=1024, out_dim=4, dim_mult=[1, 2, 4, 4], num_heads=8, head_dim=64, num_res_blocks=2,
               attn_scales=[1.0, 0.5, 0.25], camera_dim=16, use_camera_condition=True, use_fps_condition=False)
    sd = {k: torch.zeros(s) for k, s in param_shapes(cfg).items()}
    dev = torch.device("cpu")
    e64 = UNetEngine(cfg, sd, 2, 24, 40, 64, 77, dev, n_t=1, share_prefix=True)
    e32 = UNetEngine(cfg, sd, 2, 24, 32, 32, 77, dev, n_t=1, share_prefix=True, packed=e64.packed)
    assert e64.S.nops == 766
    want = {e64: [(7680, 1280, 5120), (30720, 1280, 5120), (122880, 640, 2560)],
            e32: [(12288, 1280, 5120), (49152, 640, 2560)]}
    for eng in (e64, e32):
        ph = _phased(eng)
        assert [(p.M, p.N, p.ktot) for _, p in ph] == want[eng]
        for lb, p in ph:
            assert eng.S.lib.vmv_gemm_validate(ctypes.byref(p)) == 0, lb
            assert eng.S.lib.vmv_gemm_pick_tile(ctypes.byref(p)) in (20, 21, 22) and "u1p" in ops.gemm_signature(p)
        nine = [(p.M, p.N, p.ktot) for op, p in eng.S.recorded if op == 1 and "u1F" in ops.gemm_signature(p)]      # nine-tap up convolutions left
        assert nine == ([] if eng is e64 else [(3072, 1280, 11520)])


def test_validate_refuses_everything_else_that_sets_the_field():
    from videomv_amd import _lib as L, ops
    lib = L.load()
    n, IH, IW, Cc, N = 2, 3, 5, 16, 8
    x = torch.zeros(n * IH * IW, Cc, dtype=L.elem())
    x2 = torch.zeros(n * IH * IW, Cc, dtype=L.elem())
    W4 = torch.zeros(4 * N, 4 * Cc, dtype=L.elem())
    out = torch.zeros(4 * n * IH * IW, N, dtype=L.elem())
    res = torch.zeros(4 * n * IH * IW, N, dtype=L.elem())
    rv = torch.zeros(4 * n, N)
    ws = torch.zeros(2 * 4 * n * IH * IW * N)
    M = 4 * n * IH * IW

    def build(segs=None, geom=None, **kw):
        return ops.gemm_params(M, N, segs or ops.up4_segs(x, Cc, Cc), W4, out, N, phased=True,
                               geom=geom or ops.Geom(OH=2 * IH, OW=2 * IW, IH=IH, IW=IW, stride=1, ups=1), **kw)
    ok = lambda p: lib.vmv_gemm_validate(ctypes.byref(p))
    assert ok(build()) == 0
    assert ok(build(tile=L.TILE_X256x128)) == 0 and ok(build(tile=L.TILE_X256x320)) == 0
    bad = [build(residual=res, ldr=N), build(rowvec=rv, rowvec_div=IH * IW * 4, rowvec_ld=N),
           build(segs=ops.conv3x3_segs([(x, Cc, Cc)])[:4]),                                                       # taps other than the four
           build(segs=list(reversed(ops.up4_segs(x, Cc, Cc)))),                                                   # ... or in another order
           build(geom=ops.Geom(OH=2 * IH, OW=2 * IW, IH=IH, IW=IW, stride=1, ups=0)),                             # ups == 0
           build(segs=ops.up4_segs(x, Cc, Cc)[:2] + ops.up4_segs(x2, Cc, Cc)[2:]),                                # two sources
           build(out_fp32=True), build(epilogue=L.EPI_GEGLU), build(ksplit=2, workspace=ws),
           build(geom=ops.Geom(OH=IH, OW=IW, IH=IH, IW=IW, stride=1, ups=1)),
           build(tile=L.TILE_256x128), build(tile=L.TILE_128x128), build(tile=L.TILE_X512x128)]                  # no serving kernel
    for i, p in enumerate(bad):
        assert ok(p) == -1, i
    # the predicate: the size rule on top of the validation (default: more than 768 rows per phase)
    assert lib.vmv_gemm_up4_ok(ctypes.byref(build())) == 0
    nine = ops.gemm_params(M, N, ops.conv3x3_segs([(x, Cc, Cc)]), torch.zeros(N, 9 * Cc, dtype=L.elem()), out, N,
                           geom=ops.Geom(OH=2 * IH, OW=2 * IW, IH=IH, IW=IW, stride=1, ups=1))
    assert ok(nine) == 0 and lib.vmv_gemm_up4_ok(ctypes.byref(nine)) == 0
