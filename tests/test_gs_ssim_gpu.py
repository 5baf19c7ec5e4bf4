"""L1 + D-SSIM loss on the GPU (csrc/gs_ssim.hip through vmv_gs_ssim_loss and videomv_amd.gs_fit): the kernel's scalars and gradient
against the fp64 yardstick (tests/ssim_ref.py) under a tolerance taken from the yardstick's own fp32 error, forward-only mode and
determinism, the untouched MSE default, the loss inside the fitter's chain, convergence against the MSE fit, and the t2v entrance."""
import ctypes as C
import math
import os

import pytest
import torch

from tests import ssim_ref as R
from tests.test_gs_fit_gpu import FOVY, _cams, _entrance_cfg, _orbit_scene, _rel, _scene

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 0.2, 1.0)
ULP = 2.0 ** -24


def _run(img, tgt, lam, grad=True):
    """vmv_gs_ssim_loss on GPU tensors [P, H, W] -> (3 scalars as a CPU fp32 tensor, dL/dimage or None)"""
    from videomv_amd import _lib as L
    from videomv_amd.gs_fit import ssim_loss_params, ssim_workspace
    from videomv_amd.ops import _stream_ptr
    P, H, W = img.shape
    ws = ssim_workspace(P, H, W, img.device)
    out = torch.zeros(3, dtype=torch.float32, device=img.device)
    dl = torch.full_like(img, float("nan")) if grad else None
    L.check(L.load().vmv_gs_ssim_loss(C.byref(ssim_loss_params(img, tgt, lam, dl, out, ws)), _stream_ptr()), "gs_ssim_loss")
    torch.cuda.synchronize()
    return out.cpu(), dl


def _smooth(planes, size, coarse, gen):
    x = torch.rand(planes, 1, coarse, coarse, generator=gen)
    return torch.nn.functional.interpolate(x, size=(size, size), mode="bicubic", align_corners=False)[:, 0].clamp(0, 1).contiguous()


def _inputs(kind):
    """fp32 CPU pairs [P, H, W] in [0, 1]"""
    gen = torch.Generator().manual_seed({"noise": 1, "smooth": 2, "near": 3, "tiny": 4, "production": 5}[kind])
    if kind == "noise":                      # tile tails in both directions
        return torch.rand(9, 37, 41, generator=gen), torch.rand(9, 37, 41, generator=gen)
    if kind == "smooth":                     # like renders
        return _smooth(6, 64, 8, gen), _smooth(6, 64, 8, gen)
    if kind == "near":                       # near-identical, the left half a constant 0.5 in both: L1 ties, E[x^2] - mu^2 cancellation
        tgt = _smooth(6, 64, 8, gen)
        img = (tgt + 0.01 * (torch.rand(6, 64, 64, generator=gen) - 0.5)).clamp(0, 1)
        img[:, :, :32] = 0.5
        tgt[:, :, :32] = 0.5
        return img.contiguous(), tgt.contiguous()
    if kind == "tiny":                       # smaller than the window
        return torch.rand(3, 7, 9, generator=gen), torch.rand(3, 7, 9, generator=gen)
    return _smooth(72, 256, 32, gen), _smooth(72, 256, 32, gen)      # the production shape: 24 views x 3 channels of 256 x 256


def _compare(img, tgt, lam, got_scalars, got_grad, what):
    """The issue's tolerance rule: e32 = the error of the yardstick evaluated in fp32 on the CPU against its fp64 self on the same
    numbers; the kernel's error against fp64 <= 10 e32 (gradient, relative L2) and <= max(10 e32, 64 * 2^-24) (each scalar, relative)."""
    s64, g64 = R.l1_dssim_with_grad(img.double(), tgt.double(), lam)
    s32, g32 = R.l1_dssim_with_grad(img.float(), tgt.float(), lam)
    e32_g = _rel(g32.double(), g64)
    err_g = _rel(got_grad.detach().cpu().double(), g64)
    print(f"{what} lambda={lam}: gradient rel-L2 {err_g:.3e} (fp32 yardstick {e32_g:.3e}, bound {10 * e32_g:.3e})")
    ok = err_g <= 10 * e32_g
    for name, a, b, c in zip(("objective", "L1", "SSIM"), got_scalars.tolist(), s64, s32):
        e32, err = abs(c - b) / abs(b), abs(a - b) / abs(b)
        bound = max(10 * e32, 64 * ULP)
        print(f"    {name}: {a:.9g} vs {b:.12g}: rel {err:.3e} (fp32 yardstick {e32:.3e}, bound {bound:.3e})")
        ok = ok and err <= bound
    return ok


@pytest.mark.parametrize("kind", ["noise", "smooth", "near", "tiny", "production"])
def test_kernel_matches_the_fp64_yardstick(kind):
    img, tgt = _inputs(kind)
    if kind == "near":
        assert int((img == tgt).sum()) >= 6 * 64 * 32
    a, b = img.cuda(), tgt.cuda()
    bad = []
    for lam in LAMBDAS:
        out, dl = _run(a, b, lam)
        assert torch.isfinite(dl).all()           # every pixel written (the buffer starts as NaN)
        if not _compare(img, tgt, lam, out, dl, kind):
            bad.append(lam)
    assert not bad, bad


def test_forward_only_mode_determinism_and_identity():
    img, tgt = (t.cuda() for t in _inputs("noise"))
    out, dl = _run(img, tgt, 0.2)
    out0, none = _run(img, tgt, 0.2, grad=False)
    assert none is None and torch.equal(out.view(torch.int32), out0.view(torch.int32))          # the same scalars, bit for bit
    out2, dl2 = _run(img, tgt, 0.2)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(dl.view(torch.int32), dl2.view(torch.int32))
    for kind in ("noise", "near", "production"):
        x = _inputs(kind)[0].cuda()
        same, _ = _run(x, x, 1.0, grad=False)
        print(kind, "SSIM(x, x) =", repr(float(same[2])), "L1 =", float(same[1]))
        assert abs(float(same[2]) - 1.0) <= 8 * ULP and float(same[1]) == 0.0 and abs(float(same[0])) <= 8 * ULP
    from videomv_amd.gs_fit import ssim
    x, y = _inputs("smooth")
    ref = float(R.ssim_map(x.double(), y.double()).mean())
    got = ssim(x.cuda().reshape(2, 3, 64, 64), y.cuda().reshape(2, 3, 64, 64))                 # the public metric, [..., H, W]
    assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    with pytest.raises(ValueError):
        ssim(x.cuda(), y.cuda()[:3])


def _fitter(loss, **kw):
    from videomv_amd.gs_fit import GaussianFitter
    g = _scene(300, 11)
    cv, cvp = _cams(3)
    tg_g = _scene(300, 12)
    from videomv_amd.gs import GaussianRenderer
    tg = GaussianRenderer(64, FOVY).render(tg_g.unsqueeze(0).cuda(), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None,
                                           bg_color=torch.tensor([0.5, 0.5, 0.5]))["image"][0]
    return GaussianFitter(g.cuda(), cv.cuda(), cvp.cuda(), tg, bg=(0.5, 0.5, 0.5), fovy=FOVY, loss=loss, **kw)


def test_mse_default_never_calls_the_new_entry_point(monkeypatch):
    from videomv_amd import _lib as L

    def boom(*a, **k):
        raise AssertionError("vmv_gs_ssim_loss called on the MSE path")
    monkeypatch.setattr(L.load(), "vmv_gs_ssim_loss", boom)
    st = _fitter("mse").fit(3)
    assert st["iters"] == 3 and "ssim_after" not in st and "mse_after" not in st and st["loss_after"] > 0
    assert st["psnr_after"] == pytest.approx(-10 * math.log10(st["loss_after"]), rel=1e-9)
    f = _fitter("mse")
    f._forward()
    f._loss()
    torch.cuda.synchronize()
    x = f.image.clone().requires_grad_(True)
    ref = torch.nn.functional.mse_loss(x, f.targets.reshape(x.shape))
    ref.backward()
    assert abs(float(f.loss) - float(ref.detach())) <= 1e-6 * float(ref.detach()) and _rel(f.dL.cpu().double(), x.grad.cpu().double()) < 1e-6


def test_loss_is_wired_into_the_fitters_chain():
    f = _fitter("l1_dssim", lambda_dssim=0.2)
    f._forward()
    f._loss()
    torch.cuda.synchronize()
    img, tgt = f.image.cpu().reshape(-1, 64, 64), f.targets.cpu().reshape(-1, 64, 64)
    assert img.shape[0] == 9 and float((img - tgt).abs().max()) > 0.05
    assert _compare(img, tgt, 0.2, f.loss3.cpu(), f.dL.reshape(-1, 64, 64), "fitter")
    assert float(f.loss) == float(f.loss3[0])


def test_l1_dssim_fit_converges():
    """The perturbed scene of test_fit_converges_and_stays_at_the_ground_truth (same seeds), 100 iterations, once per objective.
    Required of l1_dssim: its objective falls, SSIM and PSNR rise, and its PSNR gain is at least half the MSE run's in this same test
    (a guard against a wrong sign or scale, not a quality claim).  Measured once on an MI355X: mse 26.09 -> 37.24 dB,
    SSIM 0.86386 -> 0.97378; l1_dssim 26.09 -> 38.32 dB, SSIM 0.86386 -> 0.98266."""
    from videomv_amd.gs_fit import GaussianFitter, ssim
    gt, cv, cvp, tg = _orbit_scene()
    gen = torch.Generator().manual_seed(5)
    pert = gt.clone()
    pert[:, 0:3] += 0.01 * torch.randn(gt.shape[0], 3, generator=gen)
    pert[:, 3] = (pert[:, 3] + 0.2 * torch.randn(gt.shape[0], generator=gen)).clamp(0.05, 0.95)
    pert[:, 4:7] *= torch.exp(0.2 * torch.randn(gt.shape[0], 3, generator=gen))
    pert[:, 11:14] = (pert[:, 11:14] + 0.15 * torch.randn(gt.shape[0], 3, generator=gen)).clamp(0.02, 0.98)
    res = {}
    for loss in ("mse", "l1_dssim"):
        f = GaussianFitter(pert.cuda(), cv.cuda(), cvp.cuda(), tg, bg=(0.5, 0.5, 0.5), fovy=FOVY, loss=loss)
        f.evaluate()
        s0 = ssim(f.images(), f.targets)
        st = f.fit(100)
        f.evaluate()
        st["ssim_metric_before"], st["ssim_metric_after"] = s0, ssim(f.images(), f.targets)
        res[loss] = st
        print(f"{loss}: PSNR {st['psnr_before']:.2f} -> {st['psnr_after']:.2f} dB, SSIM {s0:.5f} -> {st['ssim_metric_after']:.5f}, "
              f"objective {st['loss_before']:.4e} -> {st['loss_after']:.4e}")
    m, d = res["mse"], res["l1_dssim"]
    assert d["ssim_before"] == pytest.approx(d["ssim_metric_before"], abs=1e-6) and d["ssim_after"] == pytest.approx(d["ssim_metric_after"], abs=1e-6)
    assert d["loss_after"] < d["loss_before"] and d["ssim_after"] > d["ssim_before"] and d["psnr_after"] > d["psnr_before"]
    gain_m, gain_d = m["psnr_after"] - m["psnr_before"], d["psnr_after"] - d["psnr_before"]
    assert gain_m > 8.0                                   # the parent's path, as test_fit_converges_and_stays_at_the_ground_truth
    assert gain_d >= 0.5 * gain_m, (gain_d, gain_m)


def test_t2v_entrance_fits_with_l1_dssim(tmp_path):
    from videomv_amd.registry import INFER_ENGINE
    from videomv_amd.gs import GaussianRenderer
    import videomv_amd.entrance  # noqa: F401
    runs = {}
    for name, extra in (("plain", []), ("export", ["save_gaussians", "True", "gs_fit_iters", "20", "gs_fit_loss", "l1_dssim"])):
        cu = _entrance_cfg(tmp_path / name, extra)
        runs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    cfg = runs["export"]
    assert len(cfg.gs_exports) == 2
    for e in cfg.gs_exports:
        g = GaussianRenderer.load_ply(e["ply"])
        assert 0 < g.shape[0] <= 64 * 64 * 4 and torch.isfinite(g).all()
        assert e["loss_after"] < e["loss_before"] and 0 < e["ssim_after"] <= 1 and 0 < e["ssim_before"] <= 1
        assert e["psnr_after"] == pytest.approx(-10 * math.log10(e["mse_after"]), rel=1e-9)
    for a, b in zip(sorted(runs["plain"].outputs), sorted(cfg.outputs)):
        assert os.path.basename(a) == os.path.basename(b)
        for suffix in (".pt", "_gs.pt"):
            pa, pb = torch.load(a.replace(".pt", suffix)), torch.load(b.replace(".pt", suffix))
            assert torch.equal(pa["latent"], pb["latent"])
