"""TEST INFRASTRUCTURE (CPU): the rasteriser's blend restated in fp64 with depth in it, over ``oracle.gs_ref.preprocess``.

Written from the definitions of include/vmv.h (vmv_gs_batch_render_depth), not from the kernel.  Per pixel, over the Gaussians whose
tile rectangle holds the pixel's 16 x 16 tile, front to back by (view depth, index):
  power = -0.5 (A dx^2 + C dy^2) - B dx dy ; skipped if power > 0 ; alpha = min(0.99, o e^power) ; skipped if alpha < 1/255 ;
  the pixel stops BEFORE the Gaussian that would take T below 1e-4 ; otherwise the Gaussian is APPLIED: w = alpha T, T <- T (1 - alpha).
  D      = sum w z                                      expected depth, not normalised
  median = z of the first applied Gaussian after which T < 0.5, else 0
  margin = min |T_after - 0.5| over the applied Gaussians (0.5 if none: T stays 1) — how far the pixel is from a different answer
The preprocess runs in fp32 like the oracle's (the same rectangles, radii and depths as ``oracle.gs_ref.render``); the blend is fp64 and
vectorised over pixels x Gaussians (the oracle's loop takes one Gaussian at a time); image and alpha come out of the same weights, so
the CPU tests can hold the whole restatement against the oracle.  ``pos`` / ``count`` describe the staging the
kernel does: the 0-based position of the median Gaussian in its tile's instance list (-1 without a median) and the length of that list.
"""
import math

import torch

from oracle.gs_ref import TILE, preprocess


@torch.no_grad()
def blend_depth(gaussians, view, view_proj, size, tan_half_fov, bg=None, rows_per_chunk=None):
    """gaussians [N, 14], one view -> dict of [size, size] maps: D, median, margin, alpha (fp64), has (bool), pos, count (int64),
    image [3, size, size] (fp64, over the background ``bg`` [3], default 0; not clamped) and z_max = the largest valid view depth."""
    g = gaussians.float()
    pp = preprocess(g[:, 0:3], g[:, 4:7], g[:, 7:11], view.float(), view_proj.float(), size, tan_half_fov)
    idx = torch.nonzero(pp["valid"]).flatten()
    order = idx[torch.argsort(pp["depth"][idx], stable=True)]
    G = int(order.numel())
    bg = torch.zeros(3, dtype=torch.float64) if bg is None else bg.double().cpu()
    out = dict(image=bg.view(3, 1, 1).expand(3, size, size).clone(), alpha=torch.zeros(size, size, dtype=torch.float64),
               D=torch.zeros(size, size, dtype=torch.float64), median=torch.zeros(size, size, dtype=torch.float64),
               margin=torch.full((size, size), 0.5, dtype=torch.float64), has=torch.zeros(size, size, dtype=torch.bool),
               pos=torch.full((size, size), -1, dtype=torch.int64), count=torch.zeros(size, size, dtype=torch.int64),
               z_max=float(pp["depth"][idx].max()) if G else 0.0)
    if G == 0:
        return out
    x, y = pp["xy"][order, 0].double(), pp["xy"][order, 1].double()
    A, B, Cc = (pp["conic"][order, i].double() for i in range(3))
    o, z, rgb = g[order, 3].double(), pp["depth"][order].double(), g[order, 11:14].double()
    x0, y0, x1, y1 = (pp["rect"][order, i] for i in range(4))
    rows = rows_per_chunk or max(1, min(size, (1 << 22) // max(1, G * size)))
    for r0 in range(0, size, rows):
        r1 = min(size, r0 + rows)
        ys, xs = torch.meshgrid(torch.arange(r0, r1), torch.arange(size), indexing="ij")
        ys, xs = ys.reshape(-1, 1), xs.reshape(-1, 1)
        tx, ty = xs // TILE, ys // TILE
        in_rect = (tx >= x0) & (tx < x1) & (ty >= y0) & (ty < y1)                     # [P, G]
        dx, dy = x - xs.double(), y - ys.double()
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        alpha = torch.clamp(o * torch.exp(power), max=0.99)
        hit = in_rect & (power <= 0) & (alpha >= 1.0 / 255.0)
        keep = torch.where(hit, 1.0 - alpha, torch.ones_like(alpha))
        T_before = torch.cat([torch.ones_like(keep[:, :1]), torch.cumprod(keep, dim=1)[:, :-1]], dim=1)      # exclusive product
        T_after = T_before * (1.0 - alpha)
        stop = hit & (T_after < 1e-4)
        apply = hit & (torch.cumsum(stop.long(), dim=1) == 0)                          # up to, not including, the first stop
        w = torch.where(apply, alpha * T_before, torch.zeros_like(alpha))
        cross = apply & (T_after < 0.5)
        has = cross.any(dim=1)
        first = torch.argmax(cross.long(), dim=1)
        position = torch.cumsum(in_rect.long(), dim=1).gather(1, first.unsqueeze(1)).squeeze(1) - 1
        gap = torch.where(apply, (T_after - 0.5).abs(), torch.full_like(alpha, 0.5)).min(dim=1).values
        sh = (r1 - r0, size)
        T_final = torch.where(apply, 1.0 - alpha, torch.ones_like(alpha)).prod(dim=1)
        out["image"][:, r0:r1] = (w @ rgb + T_final.unsqueeze(1) * bg).t().reshape(3, *sh)
        out["alpha"][r0:r1] = w.sum(dim=1).view(sh)
        out["D"][r0:r1] = (w * z).sum(dim=1).view(sh)
        out["median"][r0:r1] = torch.where(has, z[first], torch.zeros_like(gap)).view(sh)
        out["margin"][r0:r1] = gap.view(sh)
        out["has"][r0:r1] = has.view(sh)
        out["pos"][r0:r1] = torch.where(has, position, torch.full_like(position, -1)).view(sh)
        out["count"][r0:r1] = in_rect.sum(dim=1).view(sh)
    return out


def blend_depth_views(gaussians, cam_view, cam_view_proj, size, fovy_deg, bg=None):
    """gaussians [N, 14], cam_* [V, 4, 4] -> one ``blend_depth`` dict per view."""
    tan = math.tan(0.5 * math.radians(fovy_deg))
    return [blend_depth(gaussians, cam_view[v], cam_view_proj[v], size, tan, bg) for v in range(cam_view.shape[0])]


def staging_scene(size=32, fovy_deg=39.6, n=900, seed=7, sigma_px=0.6):
    """For an identity camera at ``size`` px: ``n`` small, faint isotropic Gaussians (screen sigma ``sigma_px`` before the 0.3 dilation,
    opacity 0.08 .. 0.16, depth 1 .. 2) with centres spread over tile (0, 0) — that tile's instance list is longer than two staging
    batches of 256 and most pixels that reach T < 0.5 do so deep into it.  -> gaussians [n, 14] (the caller asserts those facts)."""
    tan = math.tan(0.5 * math.radians(fovy_deg))
    f = size / (2 * tan)
    g = torch.Generator().manual_seed(seed)
    z = 1.0 + torch.rand(n, generator=g)
    px = 1.0 + 13.0 * torch.rand(n, 2, generator=g)
    xy = ((2 * px + 1) / size - 1) * tan * z[:, None]
    s = (sigma_px * z / f)[:, None].expand(n, 3)
    o = 0.08 + 0.08 * torch.rand(n, 1, generator=g)
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(n, 4)
    return torch.cat([xy, z[:, None], o, s, rot, torch.rand(n, 3, generator=g)], dim=1)


AMBIGUOUS_MARGIN, AMBIGUOUS_CAP = 1e-4, 0.01


def compare_view(depth, median, ref, label=""):
    """One view of the rasteriser's depth outputs ([S, S] fp32) against ``blend_depth``'s dict; prints every figure, then asserts:
    expected depth over z_max held to the rasteriser's colour-channel bound (tests/test_gs_gpu.py: mean |error| < 2e-4, fewer than 0.2 %
    of pixels off by more than 2e-3); pixels whose reference margin is below 1e-4 are ambiguous (at most 1 % of the view) and left out of
    the median comparison; of the others all but 0.2 % agree on having a median and on its value to 1e-5 z_max (fp32 rounding of the view
    transform: 2^-24 relative per operation, a handful of operations)."""
    zm = ref["z_max"] if ref["z_max"] > 0 else 1.0
    d = (depth.double().cpu() - ref["D"]).abs() / zm
    amb = ref["margin"] < AMBIGUOUS_MARGIN
    med = median.double().cpu()
    bad = ((med > 0) != ref["has"]) | ((med - ref["median"]).abs() > 1e-5 * zm)
    clear = int((~amb).sum())
    fig = dict(depth_mean=float(d.mean()), depth_off=float((d > 2e-3).double().mean()), ambiguous=float(amb.double().mean()),
               median_bad=float((bad & ~amb).sum()) / max(1, clear), with_median=float(ref["has"].double().mean()))
    print(f"gs depth {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    assert torch.isfinite(depth).all() and torch.isfinite(median).all()
    assert fig["ambiguous"] <= AMBIGUOUS_CAP, fig
    assert fig["depth_mean"] < 2e-4 and fig["depth_off"] < 2e-3, fig
    assert fig["median_bad"] < 2e-3, fig
    return fig
