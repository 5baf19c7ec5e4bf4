"""The phased nearest-x2 + 3x3 convolution (include/vmv.h: VmvGemmParams.phased; csrc/gemm_xglds.hip UP4) on the GPU: every tile that
serves the mode against (a) the contract — fp32 matmuls on the same 16-bit rows and the same packed 16-bit phase weights — and (b) the
fp32 convolution of the up-sampled image, beside the nine-tap launch on the same inputs; then a small UNet forward with the mode on and off."""
import ctypes as C
import dataclasses

import pytest
import torch
import torch.nn.functional as Fn

from videomv_amd import _lib as L
from videomv_amd import ops, packing as P
from tests import up4_ref
from tests.test_kernels_gpu import BF, check, g, rel_l2, rnd

pytestmark = pytest.mark.gpu

UP4_TILES = [0, L.TILE_X256x320, L.TILE_X256x256, L.TILE_X256x128]      # auto + every tile id that claims the mode
# (n, IH, IW, C, N): Mp = 105 — four ragged single-tile phases, odd sizes, both borders in every tile; Mp = 320 — two 256-row tiles per phase,
# the second ragged, C no multiple of the 32-deep chunk, N no tile multiple; one-pixel-wide images; Mp = 1024 — whole tiles, several chunks per
# tap in the run-wise walk, the 320-column tile
CASES = [(3, 5, 7, 64, 128), (2, 10, 16, 72, 136), (2, 1, 9, 64, 64), (2, 9, 1, 64, 64), (4, 16, 16, 320, 320)]
_REF = {}


def _case(n, IH, IW, Cc, N):
    """Inputs and the two references of a case, computed once and shared by the tiles."""
    key = (n, IH, IW, Cc, N)
    if key not in _REF:
        x = rnd((n * IH * IW, Cc), 1)
        w = torch.randn(N, Cc, 3, 3, generator=g(2)) * (9 * Cc) ** -0.5
        b = torch.randn(N, generator=g(3))
        w4 = P.pack_conv3x3_up4(w, "cpu")
        w9 = P.pack_conv3x3(w, "cpu")
        contract = up4_ref.up4_rows(x.float(), n, IH, IW, w4.float().view(4, N, 4 * Cc), b)
        img = x.float().view(n, IH, IW, Cc).permute(0, 3, 1, 2)
        conv = Fn.conv2d(Fn.interpolate(img, scale_factor=2, mode="nearest"), w, b, padding=1).permute(0, 2, 3, 1).reshape(4 * n * IH * IW, N)
        _REF[key] = dict(x=x, b=b, w4=w4, w9=w9, contract=contract, conv=conv)
    return _REF[key]


def _launch(c, n, IH, IW, Cc, N, tile, phased):
    x, b = c["x"].cuda(), c["b"].cuda()
    w = (c["w4"] if phased else c["w9"]).cuda()
    M = 4 * n * IH * IW
    out = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    segs = ops.up4_segs(x, Cc, Cc) if phased else ops.conv3x3_segs([(x, Cc, Cc)])
    p = ops.gemm_params(M, N, segs, w, out, N, bias=b, geom=ops.Geom(OH=2 * IH, OW=2 * IW, IH=IH, IW=IW, stride=1, ups=1), tile=tile, phased=phased)
    ops.Stream(record=False).gemm(p, "up4" if phased else "up9")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("tile", UP4_TILES)
@pytest.mark.parametrize("n,IH,IW,Cc,N", CASES)
def test_gemm_up4(n, IH, IW, Cc, N, tile):
    c = _case(n, IH, IW, Cc, N)
    out = _launch(c, n, IH, IW, Cc, N, tile, True)
    # (a) the contract, at the tolerance of test_gemm_conv3x3
    check(out, c["contract"])
    # (b) as accurate as the nine-tap form against the fp32 convolution of the up-sampled image (the nine-tap launch: policy tile)
    if "e9" not in c:
        c["e9"] = rel_l2(_launch(c, n, IH, IW, Cc, N, 0, False), c["conv"])
    e4 = rel_l2(out, c["conv"])
    print(f"up4 {n}x{IH}x{IW} C={Cc} N={N} tile={tile}: rel-L2 vs fp32 conv: phased {e4:.3e}, nine-tap {c['e9']:.3e}, ratio {e4 / c['e9']:.3f}")
    assert e4 <= 1.5 * c["e9"], (e4, c["e9"])


def test_gemm_up4_has_no_split_k():
    """The phased form runs its four taps as one run of the tap-interleaved K walk; split-K walks segment-major and is refused for it
    (so there is no split-K case above)."""
    n, IH, IW, Cc, N = 4, 16, 16, 320, 320
    c = _case(n, IH, IW, Cc, N)
    x, w = c["x"].cuda(), c["w4"].cuda()
    out = torch.zeros(4 * n * IH * IW, N, dtype=BF, device="cuda")
    ws = torch.zeros(2 * out.numel(), device="cuda")
    for tile in UP4_TILES:
        p = ops.gemm_params(4 * n * IH * IW, N, ops.up4_segs(x, Cc, Cc), w, out, N, geom=ops.Geom(OH=2 * IH, OW=2 * IW, IH=IH, IW=IW, stride=1, ups=1),
                            tile=tile, phased=True, ksplit=2, workspace=ws)
        assert L.load().vmv_gemm_validate(C.byref(p)) == -1


def test_unet_forward_with_and_without_the_phased_form(monkeypatch):
    """A small UNet forward with the up convolution phased (VMV_UP4_MIN_ROWS=1) and nine-tap (a minimum no launch reaches): both inside the
    oracle tolerance of tests/test_unet_gpu.py; their distance (rounding-level: the summed weights are rounded once) is printed."""
    from oracle.unet_ref import UNetCfg, unet_forward
    from oracle.weights import random_state_dict, unet_param_shapes
    from videomv_amd.unet_engine import UNetEngine
    from tests.test_unet_gpu import TOL_FWD
    cfg = dict(in_dim=4, dim=64, context_dim=1024, out_dim=4, dim_mult=[1, 2], num_heads=2, head_dim=64, num_res_blocks=1, attn_scales=[1.0, 0.5],
               camera_dim=16, use_camera_condition=True, use_fps_condition=False)
    ocfg = UNetCfg(**{k: v for k, v in cfg.items() if k in {f.name for f in dataclasses.fields(UNetCfg)}})
    sd = random_state_dict(unet_param_shapes(ocfg), 99)
    B, F_, H, W, Lc = 2, 4, 10, 14, 77
    gen = torch.Generator().manual_seed(5)
    x, t = torch.randn(B, 4, F_, H, W, generator=gen), torch.tensor([501, 21])
    y, cam = torch.randn(B, Lc, 1024, generator=gen), torch.randn(B, F_, 16, generator=gen)
    ref = unet_forward(sd, ocfg, x, t, y, cam)
    eps = {}
    for mode, min_rows in (("phased", "1"), ("nine-tap", str(1 << 30))):
        monkeypatch.setenv("VMV_UP4_MIN_ROWS", min_rows)
        eng = UNetEngine(cfg, sd, B, F_, H, W, Lc, torch.device("cuda"), n_t=B)
        n_ph = sum(1 for op, p in eng.S.recorded if op == L.OP_GEMM and p.phased)
        assert n_ph == (1 if mode == "phased" else 0)
        eng.set_context(y.cuda()); eng.set_camera(cam.cuda())
        eng.forward_rows(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        eps[mode] = eng.eps_ncfhw().float().cpu()
        assert rel_l2(eps[mode], ref) < TOL_FWD, (mode, rel_l2(eps[mode], ref))
    print(f"UNet eps: phased vs oracle {rel_l2(eps['phased'], ref):.3e}, nine-tap vs oracle {rel_l2(eps['nine-tap'], ref):.3e}, "
          f"phased vs nine-tap {rel_l2(eps['phased'], eps['nine-tap']):.3e}")
