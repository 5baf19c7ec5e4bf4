"""The rasteriser's depth outputs without a GPU: the fp64 reference the GPU tests compare against (tests/gs_depth_ref.py) checked
against the oracle and on hand-built cases, the ABI of vmv_gs_batch_render_depth, the unprojection and the point-cloud writer, and the
entrance keys gs_orbit_depth / gs_points on the CPU plan interpreter."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

from tests import plan_interp
from tests.gs_depth_ref import blend_depth, blend_depth_views, staging_scene
from tests.test_gs_export_cpu import _files, _tiny_cfg
from tests.test_gs_gpu import _cams, _scene

FOVY = 39.6
TAN = math.tan(0.5 * math.radians(FOVY))


def test_reference_agrees_with_the_oracle():
    """D, alpha and the image of the fp64 restatement against oracle.gs_ref.render (fp32, one Gaussian at a time) on a seeded scene:
    the two differ by the oracle's fp32 rounding — a sum of at most ~100 weights of total <= 1, each rounded to 2^-24 relative, so
    1e-5 (of z_max for D) bounds it with room — except where a decision (1 / 255, T stop) falls the other way in fp32, the boundary
    pixels the rasteriser's own test allows 0.2 % of."""
    from oracle.gs_ref import render
    g = _scene(600, 21)
    cv, cvp = _cams(2)
    bg = torch.tensor([0.2, 0.5, 0.9])
    for v, ref in enumerate(blend_depth_views(g, cv, cvp, 48, FOVY, bg)):
        img, alpha, D = render(g[:, 0:3], g[:, 3:4], g[:, 4:7], g[:, 7:11], g[:, 11:14], cv[v], cvp[v], 48, TAN, bg)
        for name, a, b, scale in (("D", D[0], ref["D"], ref["z_max"]), ("alpha", alpha[0], ref["alpha"], 1.0), ("image", img, ref["image"], 1.0)):
            d = (a.double() - b).abs() / scale
            print(f"view {v} {name}: max {float(d.max()):.2e}")
            assert float((d > 1e-5).double().mean()) < 2e-3, (name, float(d.max()))
        assert 0.2 < float(ref["has"].double().mean()) and float(ref["D"].max()) > 0.5


def _axis_pair(o_front, o_back, z_front=1.2, z_back=1.8):
    """two isotropic Gaussians on the optical axis of an identity camera, 64 px"""
    rows = [[0.0, 0.0, z, o, 0.05, 0.05, 0.05, 1.0, 0.0, 0.0, 0.0, 0.5, 0.5, 0.5] for z, o in ((z_back, o_back), (z_front, o_front))]
    from videomv_amd.gs import GaussianRenderer
    r = GaussianRenderer(output_size=64)
    return blend_depth(torch.tensor(rows), torch.eye(4), r.proj_matrix, 64, r.tan_half_fov)


def test_reference_median_on_two_gaussians():
    f = 64 / (2 * TAN)
    at = lambda o, z: o * math.exp(-0.5 * 0.5 / ((f * 0.05 / z) ** 2 + 0.3))      # alpha at pixel (32, 32), half a pixel off the centre
    ref = _axis_pair(0.9, 0.1)                                       # opaque in front of faint: the front one's z
    assert at(0.9, 1.2) > 0.5 and float(ref["median"][32, 32]) == pytest.approx(1.2, abs=1e-6) and int(ref["pos"][32, 32]) == 0
    a0, a1 = at(0.9, 1.2), at(0.1, 1.8)
    assert float(ref["D"][32, 32]) == pytest.approx(1.2 * a0 + 1.8 * a1 * (1 - a0), abs=1e-6)
    assert float(ref["margin"][32, 32]) == pytest.approx(min(abs(1 - a0 - 0.5), abs((1 - a0) * (1 - a1) - 0.5)), abs=1e-6)
    ref = _axis_pair(0.3, 0.1)                                       # both faint: T stays above 0.5
    assert float(ref["median"].abs().max()) == 0.0 and not bool(ref["has"].any()) and float(ref["D"][32, 32]) > 0.3
    ref = _axis_pair(0.4, 0.4)                                       # the second one crosses: 0.6 x 0.6 < 0.5
    assert float(ref["median"][32, 32]) == pytest.approx(1.8, abs=1e-6) and int(ref["pos"][32, 32]) == 1
    assert float(ref["median"][0, 0]) == 0.0 and float(ref["D"][0, 0]) == 0.0      # far from both: nothing blends


def test_staging_scene_facts():
    """what tests/test_gs_depth_gpu.py's staging test relies on, from the reference alone"""
    from videomv_amd.gs import GaussianRenderer
    r = GaussianRenderer(output_size=32)
    ref = blend_depth(staging_scene(), torch.eye(4), r.proj_matrix, 32, r.tan_half_fov)
    clear = ref["has"] & (ref["margin"] >= 1e-4)
    assert int(ref["count"].max()) > 512 and int((clear & (ref["pos"] >= 256)).sum()) > 50 and int((clear & (ref["pos"] >= 512)).sum()) > 5
    assert float((ref["margin"] < 1e-4).double().mean()) <= 0.01


def test_depth_params_abi():
    from videomv_amd import _lib as L
    lib = L.load()
    assert lib.vmv_abi_version() == L.ABI_VERSION == 12
    assert lib.vmv_sizeof(108) == C.sizeof(L.GsDepthParams) == C.sizeof(L.GsBatchParams) + 16
    assert L.GsDepthParams.pass_.offset == 0 and L.GsDepthParams.out_depth.offset == C.sizeof(L.GsBatchParams)
    p = L.GsDepthParams()
    assert lib.vmv_gs_batch_render_depth(None, None) == -3           # VMV_ENULL, before anything touches a device
    assert lib.vmv_gs_batch_render_depth(C.byref(p), None) == -3     # null out_depth
    keep = torch.zeros(4)
    p.out_depth = keep.data_ptr()
    assert lib.vmv_gs_batch_render_depth(C.byref(p), None) == -3     # out_depth given: now the checks of `pass` (all null)


@pytest.mark.parametrize("size", [64, 40])
def test_depth_to_points_returns_projected_points(size):
    """World points projected with the renderer's own cam_view / proj_matrix to the pixel grid: points chosen ON pixel centres, their
    exact view depth written into a depth map, come back to 1e-5."""
    from videomv_amd.gs import GaussianRenderer, depth_to_points
    r = GaussianRenderer(output_size=size)
    cv, cvp = _cams(3)
    gen = torch.Generator().manual_seed(3)
    for v in range(3):
        ys, xs = torch.randperm(size, generator=gen)[:12], torch.randperm(size, generator=gen)[:12]
        z = 1.0 + torch.rand(12, generator=gen)
        ndc = torch.stack([(2 * xs + 1) / size - 1, (2 * ys + 1) / size - 1], dim=1).double()
        pv = torch.cat([ndc * r.tan_half_fov * z.double()[:, None], z.double()[:, None], torch.ones(12, 1, dtype=torch.float64)], dim=1)
        world = (pv @ torch.inverse(cv[v].double()))[:, :3]
        # the forward direction, independently: through cam_view_proj and the rasteriser's pixel formula
        hom = torch.cat([world, torch.ones(12, 1, dtype=torch.float64)], dim=1) @ cvp[v].double()
        pix = ((hom[:, :2] / hom[:, 3:4] + 1) * size - 1) / 2
        assert torch.allclose(pix, torch.stack([xs, ys], dim=1).double(), atol=1e-4)
        zv = (torch.cat([world, torch.ones(12, 1, dtype=torch.float64)], dim=1) @ cv[v].double())[:, 2]
        depth = torch.zeros(size, size)
        depth[ys, xs] = zv.float()
        pts, idx = depth_to_points(depth, cv[v], r.tan_half_fov)
        assert pts.shape == (12, 3) and torch.equal(idx, torch.sort(ys * size + xs).values)
        order = torch.argsort(ys * size + xs)
        assert float((pts.double() - world[order]).abs().max()) < 1e-5
        half = torch.zeros(size, size, dtype=torch.bool)
        half[: size // 2] = True
        pts_h, idx_h = depth_to_points(depth, cv[v], r.tan_half_fov, mask=half)
        assert torch.equal(idx_h, idx[idx < (size // 2) * size]) and torch.equal(pts_h, pts[: idx_h.numel()])


def test_depth_to_points_fronto_parallel_plane():
    from videomv_amd.gs import GaussianRenderer, depth_to_points
    S, z0 = 16, 1.5
    r = GaussianRenderer(output_size=S)
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.3, -0.2, -2.0])                     # camera at (0.3, -0.2, -2) looking down +z
    view = torch.inverse(c2w).transpose(0, 1)
    pts, idx = depth_to_points(torch.full((S, S), z0), view, r.tan_half_fov)
    assert pts.shape == (S * S, 3) and torch.equal(idx, torch.arange(S * S))
    assert torch.allclose(pts[:, 2], torch.full((S * S,), z0 - 2.0), atol=1e-6)
    grid = pts.view(S, S, 3)
    step = 2 * z0 * r.tan_half_fov / S                                # one pixel footprint at depth z0
    assert torch.allclose(grid[:, 1:, 0] - grid[:, :-1, 0], torch.full((S, S - 1), step), atol=1e-6)
    assert torch.allclose(grid[1:, :, 1] - grid[:-1, :, 1], torch.full((S - 1, S), step), atol=1e-6)
    assert torch.allclose(grid[..., :2].mean(dim=(0, 1)), torch.tensor([0.3, -0.2]), atol=1e-6)      # symmetric about the axis


def test_points_ply_round_trip_and_voxel_merge(tmp_path):
    from videomv_amd.gs import load_points_ply, merge_points_voxel, save_points_ply
    gen = torch.Generator().manual_seed(5)
    pts, cols = torch.randn(37, 3, generator=gen), torch.rand(37, 3, generator=gen)
    path = str(tmp_path / "p.ply")
    assert save_points_ply(pts, cols, path) == 37
    with open(path, "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n")[:-1] == ["ply", "format binary_little_endian 1.0", "element vertex 37", "property float x",
                                                     "property float y", "property float z", "property uchar red", "property uchar green",
                                                     "property uchar blue"]
    assert len(body) == 37 * 15
    rows = [struct.unpack("<3f3B", body[15 * i:15 * (i + 1)]) for i in range(37)]                 # an independent reader
    assert np.array_equal(np.array([r[:3] for r in rows], dtype=np.float32), pts.numpy())
    assert np.array_equal(np.array([r[3:] for r in rows]), np.floor(cols.numpy() * 255.0 + 0.5).astype(np.int64))
    back, rgb = load_points_ply(path)
    assert torch.equal(back, pts) and rgb.dtype == torch.uint8 and float((rgb.float() / 255 - cols).abs().max()) <= 0.5 / 255 + 1e-6
    assert save_points_ply(pts[:0], cols[:0], path) == 0 and load_points_ply(path)[0].shape == (0, 3)
    # two points in one voxel become their mean (position and colour); a third, elsewhere, stays
    p = torch.tensor([[0.11, 0.12, 0.13], [0.19, 0.18, 0.17], [0.31, 0.12, 0.13]])
    c = torch.tensor([[1.0, 0.0, 0.2], [0.0, 1.0, 0.4], [0.3, 0.3, 0.3]])
    mp, mc = merge_points_voxel(p, c, 0.1)
    assert mp.shape == (2, 3)
    assert torch.allclose(mp, torch.tensor([[0.15, 0.15, 0.15], [0.31, 0.12, 0.13]]), atol=1e-6)
    assert torch.allclose(mc, torch.tensor([[0.5, 0.5, 0.3], [0.3, 0.3, 0.3]]), atol=1e-6)
    assert merge_points_voxel(p, c, 1e-3)[0].shape == (3, 3)
    q = torch.tensor([[-0.01, 0.0, 0.0], [0.01, 0.0, 0.0]])          # either side of a voxel face: floor, not truncation
    assert merge_points_voxel(q, q, 0.1)[0].shape == (2, 3)


def _install_render_depth(monkeypatch):
    """plan_interp.install routes ``render`` to the oracle; ``render_depth`` goes to the fp64 reference the same way."""
    from videomv_amd import gs as _gs
    calls = []

    def render_depth_cpu(self, gaussians, cam_view, cam_view_proj, cam_pos=None, bg_color=None):
        calls.append(tuple(cam_view.shape[:2]))
        bg = torch.ones(3) if bg_color is None else bg_color.float().cpu()
        keys = (("image", "image"), ("alpha", "alpha"), ("depth", "D"), ("median_depth", "median"))
        out = {k: [] for k, _ in keys}
        for b in range(gaussians.shape[0]):
            refs = blend_depth_views(gaussians[b].float().cpu(), cam_view[b].float().cpu(), cam_view_proj[b].float().cpu(), self.size, self.fovy, bg)
            for k, rk in keys:
                maps = torch.stack([r[rk].float() for r in refs])
                out[k].append(maps.clamp(0, 1) if k == "image" else maps.unsqueeze(1))
        return {k: torch.stack(v) for k, v in out.items()}

    monkeypatch.setattr(_gs.GaussianRenderer, "render_depth", render_depth_cpu)
    return calls


GEOMETRY = ["gs_orbit_views", "3", "gs_orbit_size", "32", "gs_orbit_depth", "True", "gs_points", "True"]


@pytest.mark.parametrize("extra", [["gs_orbit_depth", "True", "gs_orbit_views", "3"], ["gs_points", "True", "gs_orbit_views", "3"],
                                   ["gs_points_voxel", "0.01", "gs_orbit_views", "3"],
                                   ["save_gaussians", "True", "gs_orbit_depth", "True"], ["save_gaussians", "True", "gs_points", "True"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_points_voxel", "0.01"]])
def test_geometry_keys_are_refused_before_sampling(monkeypatch, tmp_path, extra):
    """without save_gaussians, without orbit views, or a voxel without gs_points: refused, nothing sampled, nothing written"""
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, extra)
    with pytest.raises(Exception, match="gs_orbit_depth|gs_points"):
        INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    assert not os.path.exists(tmp_path / "out")


def test_entrance_writes_depth_maps_and_a_point_cloud(monkeypatch, tmp_path):
    """save_gaussians with 3 orbit views of 32 px, gs_orbit_depth and gs_points: the orbit is rendered ONCE (render_depth, no render),
    the .npy is [3, 32, 32], the sheet and the point cloud exist and load; everything else — files and latents — is the run without
    the geometry keys."""
    plan_interp.install(monkeypatch)
    calls = _install_render_depth(monkeypatch)
    from videomv_amd import gs as _gs
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    plain_render = _gs.GaussianRenderer.render
    renders = []
    monkeypatch.setattr(_gs.GaussianRenderer, "render", lambda self, *a, **k: (renders.append(1), plain_render(self, *a, **k))[1])
    base = ["save_gaussians", "True", "gs_fit_iters", "0", "gs_orbit_views", "3", "gs_orbit_size", "32"]
    cfgs = {}
    for name, extra in (("plain", base), ("geometry", base[:4] + GEOMETRY)):
        cu = _tiny_cfg(tmp_path / name, extra)
        n0 = len(renders)
        cfgs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
        assert len(renders) - n0 == (1 if name == "plain" else 0)
    assert calls == [(1, 3)]
    plain, geo = (_files(cfgs[k].log_dir) for k in ("plain", "geometry"))
    new = [f for f in geo if f.endswith(("_gs_orbit_depth.npy", "_gs_orbit_depth.png", "_gs_points.ply"))]
    assert len(new) == 3 and [f for f in geo if f not in new] == plain
    rec, = cfgs["geometry"].gs_exports
    rec0, = cfgs["plain"].gs_exports
    assert not any(k in rec0 for k in ("orbit_depth", "orbit_depth_sheet", "points_ply", "points"))
    d = np.load(rec["orbit_depth"])
    assert d.shape == (3, 32, 32) and d.dtype == np.float32 and np.isfinite(d).all() and (d >= 0).all() and (d > 0).any()
    from PIL import Image
    sheet = np.array(Image.open(rec["orbit_depth_sheet"]))
    assert sheet.shape == (32, 96) and sheet.dtype == np.uint8
    assert (sheet[np.concatenate(list(d), axis=1) == 0] == 0).all()                   # no surface: black
    pts, rgb = _gs.load_points_ply(rec["points_ply"])
    assert rec["points"] == pts.shape[0] > 0 and rec["points"] <= int((d > 0).sum()) and torch.isfinite(pts).all()
    for f in plain:
        a, b = (os.path.join(cfgs[k].log_dir, f) for k in ("plain", "geometry"))
        if f.endswith(".pt"):
            assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"])
        elif f.endswith(".png") and "_gs_orbit" in f:
            assert np.abs(np.array(Image.open(a)).astype(int) - np.array(Image.open(b)).astype(int)).max() <= 1      # oracle vs fp64 reference
