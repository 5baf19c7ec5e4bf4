"""L1 + D-SSIM loss without a GPU: the yardstick itself (tests/ssim_ref.py) against a brute-force evaluation and the hand-derived
gradient of include/vmv.h, the argument validation of vmv_gs_ssim_loss (which runs before any launch), the config keys on the CPU
plan interpreter and the fitter's loss-name check."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import plan_interp
from tests import ssim_ref as R
from tests.test_gs_export_cpu import _tiny_cfg
from videomv_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=gen, dtype=torch.float64), torch.rand(*shape, generator=gen, dtype=torch.float64)


def _brute_conv(x, g):
    """zero-padded 11 x 11 window sums from explicit patches (unfold), no conv2d"""
    P, H, W = x.shape
    patches = torch.nn.functional.unfold(torch.nn.functional.pad(x, (5, 5, 5, 5)).unsqueeze(1), kernel_size=11)      # [P, 121, H * W]
    return (patches * torch.outer(g, g).reshape(1, 121, 1)).sum(1).reshape(P, H, W)


def _sep_conv(x, g):
    """the same convolution, separably (the form of the Definition's gradient formula)"""
    P, H, W = x.shape
    x = torch.nn.functional.conv2d(x.unsqueeze(1), g.view(1, 1, 1, 11), padding=(0, 5))
    return torch.nn.functional.conv2d(x, g.view(1, 1, 11, 1), padding=(5, 0)).squeeze(1)


def test_yardstick_is_the_definition():
    g = R.window()
    assert abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0))
    img, tgt = _pair((3, 13, 17), 0)
    m = R.ssim_map(img, img)
    assert abs(float(m.mean()) - 1.0) < 1e-14 and abs(float(m.min()) - 1.0) < 1e-13
    # brute force
    mu1, mu2 = _brute_conv(img, g), _brute_conv(tgt, g)
    s11, s22, s12 = _brute_conv(img * img, g) - mu1 ** 2, _brute_conv(tgt * tgt, g) - mu2 ** 2, _brute_conv(img * tgt, g) - mu1 * mu2
    A1, A2, B1, B2 = 2 * mu1 * mu2 + R.C1, 2 * s12 + R.C2, mu1 ** 2 + mu2 ** 2 + R.C1, s11 + s22 + R.C2
    brute = A1 * A2 / (B1 * B2)
    err = float((R.ssim_map(img, tgt) - brute).abs().max())
    print("yardstick vs brute force:", err)
    assert err < 1e-12
    # the hand-derived gradient of mean(m) (include/vmv.h) against autograd
    d11, d12 = -A1 * A2 / (B1 * B2 ** 2), 2 * A1 / (B1 * B2)
    dmu = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * A1 * A2 / (B1 ** 2 * B2) - 2 * mu1 * d11 - mu2 * d12
    hand = (_sep_conv(dmu, g) + 2 * img * _sep_conv(d11, g) + tgt * _sep_conv(d12, g)) / img.numel()
    x = img.clone().requires_grad_(True)
    R.ssim_map(x, tgt).mean().backward()
    rel = float((hand - x.grad).norm() / x.grad.norm())
    print("hand-derived gradient vs autograd:", rel)
    assert rel < 1e-10
    # and the whole objective's gradient: (1 - lambda) sign / n - lambda dSSIM, sign(0) = 0
    tie = tgt.clone()
    tie[:, :, :5] = img[:, :, :5]
    (_, l1, s), grad = R.l1_dssim_with_grad(img, tie, 0.2)
    assert 0 < s < 1 and l1 > 0 and torch.isfinite(grad).all()
    _, g0 = R.l1_dssim_with_grad(img, tie, 0.0)
    assert torch.equal(g0, torch.sign(img - tie) / img.numel()) and float((g0 == 0).sum()) >= 3 * 13 * 5


def _params(lib, planes=3, height=16, width=20, lam=0.2, short=0):
    X = 1 << 20                          # any non-null address: validation never dereferences
    nbytes = C.c_size_t(0)
    assert lib.vmv_gs_ssim_loss_workspace_bytes(planes, height, width, C.byref(nbytes)) == 0
    p = L.GsSsimLossParams()
    p.image, p.target, p.dL_dimage, p.loss, p.workspace = X, X, X, X, X
    p.planes, p.height, p.width, p.lambda_dssim, p.workspace_bytes = planes, height, width, lam, nbytes.value - short
    return p


def test_validation_needs_no_gpu():
    lib = L.load()
    p = _params(lib)
    p.image = None
    assert lib.vmv_gs_ssim_loss(C.byref(p), None) == -3                       # VMV_ENULL
    for field in ("target", "loss", "workspace"):
        p = _params(lib)
        setattr(p, field, None)
        assert lib.vmv_gs_ssim_loss(C.byref(p), None) == -3, field
    assert lib.vmv_gs_ssim_loss(None, None) == -3
    p = _params(lib)
    p.height = 0
    assert lib.vmv_gs_ssim_loss(C.byref(p), None) == -1                       # VMV_EINVAL
    for lam in (1.5, -0.1, float("nan")):
        assert lib.vmv_gs_ssim_loss(C.byref(_params(lib, lam=lam)), None) == -1, lam
    assert lib.vmv_gs_ssim_loss(C.byref(_params(lib, short=1)), None) != 0     # a workspace one byte short
    p = _params(lib)
    p.planes, p.height, p.width = 1 << 11, 1 << 10, 1 << 10                      # 2^31 pixels
    assert lib.vmv_gs_ssim_loss(C.byref(p), None) == -4                       # VMV_ERANGE
    nbytes = C.c_size_t(0)
    assert lib.vmv_gs_ssim_loss_workspace_bytes(1 << 11, 1 << 10, 1 << 10, C.byref(nbytes)) == -4
    assert lib.vmv_gs_ssim_loss_workspace_bytes(3, 16, 0, C.byref(nbytes)) == -1
    assert lib.vmv_gs_ssim_loss_workspace_bytes(3, 16, 16, None) == -3

    def ws(*a):
        assert lib.vmv_gs_ssim_loss_workspace_bytes(*a, C.byref(nbytes)) == 0
        return nbytes.value
    for base in ((1, 1, 1), (3, 7, 9), (9, 37, 41), (72, 256, 256), (2, 32, 33)):
        assert ws(*base) >= 3 * 4 * base[0] * base[1] * base[2]              # the three derivative maps fit
        for k in range(3):
            for step in (1, 31, 32):
                grown = list(base)
                grown[k] += step
                assert ws(*grown) >= ws(*base), (base, grown)


def test_ctypes_struct_has_the_c_layout():
    lib = L.load()
    assert lib.vmv_sizeof(107) == C.sizeof(L.GsSsimLossParams)
    hdr = open(os.path.join(ROOT, "include", "vmv.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} VmvGsSsimLossParams;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in L.GsSsimLossParams._fields_], names
    assert "vmv_gs_ssim_loss" in L.SYMBOLS and "vmv_gs_ssim_loss_workspace_bytes" in L.SYMBOLS


@pytest.mark.parametrize("extra", [["gs_fit_loss", "bogus"], ["gs_fit_lambda_dssim", "1.5"]])
def test_bad_loss_keys_fail_before_sampling(monkeypatch, tmp_path, extra):
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, ["save_gaussians", "True"] + extra)
    with pytest.raises(Exception, match=extra[0]):                  # (the registry re-raises as Exception)
        INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    assert not os.path.exists(tmp_path / "out")                     # nothing sampled, nothing written


def test_l1_dssim_key_without_a_fit_writes_the_ply(monkeypatch, tmp_path):
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    from videomv_amd.gs import GaussianRenderer
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, ["save_gaussians", "True", "gs_fit_loss", "l1_dssim", "gs_fit_iters", "0"])
    cfg = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    rec, = cfg.gs_exports
    g = GaussianRenderer.load_ply(rec["ply"])
    assert g.shape == (rec["vertices"], 14) and g.shape[0] > 0 and torch.isfinite(g).all()
    assert cfg.gs_fit_loss == "l1_dssim" and "ssim_after" not in rec


def test_fitter_refuses_an_unknown_loss_before_the_device_check():
    from videomv_amd.gs_fit import GaussianFitter, LOSSES
    assert LOSSES == ("mse", "l1_dssim")
    g, cam, tg = torch.zeros(4, 14), torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="bogus"):
        GaussianFitter(g, cam, cam, tg, loss="bogus")
    with pytest.raises(ValueError, match="lambda_dssim"):
        GaussianFitter(g, cam, cam, tg, loss="l1_dssim", lambda_dssim=1.5)
    with pytest.raises(RuntimeError, match="GPU"):                 # a known loss gets as far as the device check
        GaussianFitter(g, cam, cam, tg, loss="l1_dssim")
