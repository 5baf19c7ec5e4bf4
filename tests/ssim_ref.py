"""The yardstick of the L1 + D-SSIM loss (csrc/gs_ssim.hip): the definition of include/vmv.h in a dozen lines of torch — ONE grouped
conv2d with the full 11 x 11 window, padding 5 (zeros) — evaluated in the dtype of its inputs, with autograd.  Deliberately not
separable: it shares no structure with the kernel.  Images are planes [P, H, W]."""
import torch

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64):
    """the 11 taps: exp(-(i - 5)^2 / (2 * 1.5^2)), normalised in double"""
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def _conv(x, w2d):
    return torch.nn.functional.conv2d(x.unsqueeze(1), w2d.view(1, 1, 11, 11), padding=5).squeeze(1)


def ssim_map(img, tgt):
    """per-pixel SSIM m [P, H, W]"""
    g = window(img.dtype)
    w = torch.outer(g, g)
    mu1, mu2 = _conv(img, w), _conv(tgt, w)
    s11, s22, s12 = _conv(img * img, w) - mu1 * mu1, _conv(tgt * tgt, w) - mu2 * mu2, _conv(img * tgt, w) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def l1_dssim(img, tgt, lam):
    """-> (objective, L1, mean SSIM) as 0-dim tensors of the inputs' dtype"""
    l1 = (img - tgt).abs().mean()
    s = ssim_map(img, tgt).mean()
    return (1 - lam) * l1 + lam * (1 - s), l1, s


def l1_dssim_with_grad(img, tgt, lam):
    """-> ((objective, L1, SSIM) as floats, d objective / d img) by autograd, in the inputs' dtype"""
    x = img.detach().clone().requires_grad_(True)
    obj, l1, s = l1_dssim(x, tgt.detach(), lam)
    obj.backward()
    return (float(obj.detach()), float(l1.detach()), float(s.detach())), x.grad.detach()
