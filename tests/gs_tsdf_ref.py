"""The yardstick of the TSDF fusion kernel (csrc/gs_tsdf.hip): the definition of include/vmv.h ("TSDF fusion"), restated from the header
text in vectorised torch, fp64 by default.  ``dtype=torch.float32`` evaluates the SAME definition in fp32 on the CPU: its error against
fp64 is what the number format costs, and ten times that is the bound the GPU tests hold the kernel to.  Analytic depth maps of spheres
for the fusion tests.  Plain Python: no fixtures."""
import functools
import math

import torch

CLEAR = 1e-4
TAN = math.tan(0.5 * math.radians(39.6))          # the renderer's default fovy (GaussianRenderer)


def tsdf_ref(depth, colour, views, tan_half_fov, res, origin, voxel, trunc, z_min=0.05, carve=True, acc=None, dtype=torch.float64):
    """depth [V, S, S], colour [V, 3, S, S] or None, views [V, 4, 4] (row-vector convention) -> (planes [7, R, R, R] ([z][y][x]; 0 sum tsdf,
    1 W, 2 n_behind, 3..5 sum R G B, 6 Wc), margin [R, R, R]).  ``acc``: planes to continue from (not modified).  ``margin`` is the
    smallest relative distance of any of the voxel's decisions to its threshold: |frac(px + 0.5) - nearest integer| (likewise py) and,
    where the pixel has a surface, |sdf + trunc| / trunc and |sdf - trunc| / trunc, over the views with z > z_min; and |z - z_min| / z_min
    over all views.  A voxel whose margin is at least CLEAR takes the same branches in fp32."""
    V, S = int(depth.shape[0]), int(depth.shape[-1])
    R = int(res)
    depth, views = depth.to(dtype).reshape(V, S, S), views.to(dtype).reshape(V, 4, 4)
    i = torch.arange(R, dtype=dtype)
    wz, wy, wx = torch.meshgrid(origin[2] + i * voxel, origin[1] + i * voxel, origin[0] + i * voxel, indexing="ij")
    planes = torch.zeros(7, R, R, R, dtype=dtype) if acc is None else acc.to(dtype).clone()
    margin = torch.full((R, R, R), float("inf"), dtype=torch.float64)
    for v in range(V):
        m = views[v]
        xv = wx * m[0, 0] + wy * m[1, 0] + wz * m[2, 0] + m[3, 0]
        yv = wx * m[0, 1] + wy * m[1, 1] + wz * m[2, 1] + m[3, 1]
        z = wx * m[0, 2] + wy * m[1, 2] + wz * m[2, 2] + m[3, 2]
        margin = torch.minimum(margin, ((z - z_min).abs() / z_min).double())
        front = z > z_min
        zs = torch.where(front, z, torch.ones_like(z))
        px = ((xv / (zs * tan_half_fov) + 1) * S - 1) / 2
        py = ((yv / (zs * tan_half_fov) + 1) * S - 1) / 2
        fx, fy = torch.floor(px + 0.5), torch.floor(py + 0.5)
        for p in (px, py):
            off = ((p + 0.5) - torch.round(p + 0.5)).abs().double()
            margin = torch.where(front, torch.minimum(margin, off), margin)
        seen = front & (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
        ix, iy = fx.clamp(0, S - 1).long(), fy.clamp(0, S - 1).long()
        d = depth[v][iy, ix]
        surf = seen & (d > 0)
        sdf = d - z
        for edge in (sdf + trunc, sdf - trunc):
            margin = torch.where(surf, torch.minimum(margin, (edge.abs() / trunc).double()), margin)
        behind = surf & (sdf < -trunc)
        fused = surf & ~behind
        free = seen & (d == 0) & bool(carve)
        planes[2] += behind.to(dtype)
        planes[0] += torch.where(fused, torch.clamp(sdf / trunc, max=1.0), torch.zeros_like(sdf)) + free.to(dtype)
        planes[1] += fused.to(dtype) + free.to(dtype)
        if colour is not None:
            near = fused & (sdf <= trunc)
            c = colour[v].to(dtype)[:, iy, ix]
            planes[3:6] += torch.where(near, c, torch.zeros_like(c))
            planes[6] += near.to(dtype)
    return planes, margin


def sphere_depth(cam_view, S, centre, r, tan_half_fov=TAN):
    """The exact view depth z (not the ray length) of the sphere |x - centre| = r per pixel CENTRE of an S x S image, 0 where the ray
    misses: the pixel (ix, iy) looks along (tan ndc_x, tan ndc_y, 1) with ndc = (2 i + 1) / S - 1 (the rasteriser's convention,
    gs.depth_to_points).  fp64 -> [S, S]."""
    cv = cam_view.double()
    c = torch.cat([torch.tensor(list(centre), dtype=torch.float64), torch.ones(1, dtype=torch.float64)]) @ cv      # the centre in view space
    ndc = (2.0 * torch.arange(S, dtype=torch.float64) + 1.0) / S - 1.0
    dy, dx = torch.meshgrid(ndc * tan_half_fov, ndc * tan_half_fov, indexing="ij")
    # points z (dx, dy, 1): |z dir - c|^2 = r^2
    a = dx * dx + dy * dy + 1.0
    b = dx * c[0] + dy * c[1] + c[2]
    disc = b * b - a * (c[0] ** 2 + c[1] ** 2 + c[2] ** 2 - r * r)
    z = (b - torch.sqrt(disc.clamp_min(0.0))) / a
    return torch.where((disc > 0) & (z > 0), z, torch.zeros_like(z))


def spheres_depth(cam_views, S, spheres, tan_half_fov=TAN):
    """The union of spheres [(centre, r), ...] in every view: the per-pixel minimum of their depths over those that are hit -> [V, S, S]"""
    out = []
    for cv in cam_views:
        best = torch.zeros(S, S, dtype=torch.float64)
        for centre, r in spheres:
            z = sphere_depth(cv, S, centre, r, tan_half_fov)
            best = torch.where((z > 0) & ((best == 0) | (z < best)), z, best)
        out.append(best)
    return torch.stack(out)


def sphere_distance(verts, spheres):
    """distance of every vertex to the nearest of the spheres' surfaces -> [n] fp64"""
    v = verts.double()
    return torch.stack([((v - torch.tensor(list(c), dtype=torch.float64)).norm(dim=1) - r).abs() for c, r in spheres]).min(0).values


def sphere_volume(r):
    return 4.0 / 3.0 * math.pi * r ** 3


# ---------------------------------------------------------------------------------------------------------------- shared cases
HALF = 0.542                                                           # 1.6 sin 19.8 deg: the ball every _cams view at distance 1.6 sees whole
SPHERE = [((0.05, -0.03, 0.02), 0.32)]
TWO_SPHERES = [((0.17, 0.0, 0.02), 0.16), ((-0.2, 0.03, -0.05), 0.13)]


def f32(x):
    """the value a C float holds"""
    return float(torch.tensor(x, dtype=torch.float32))


def pattern_colour(V, S):
    """[V, 3, S, S] in [0, 1]: differs per view, channel and pixel, not dyadic"""
    v, c, y, x = torch.meshgrid(torch.arange(V), torch.arange(3), torch.arange(S), torch.arange(S), indexing="ij")
    return (0.5 + 0.5 * torch.sin(0.37 * x + 0.23 * y + 1.3 * c + 0.9 * v)).float()


def volume_ref(vol, depth, colour, views, tan_half_fov=TAN, dtype=torch.float64, **kw):
    """``tsdf_ref`` with the geometry of a gs_mesh.TsdfVolume as its kernel call receives it (C floats)"""
    kw["z_min"] = f32(kw.get("z_min", 0.05))
    return tsdf_ref(depth, colour, views, f32(tan_half_fov), vol.res, [f32(o) for o in vol.origin], f32(vol.voxel), f32(vol.trunc),
                    dtype=dtype, **kw)


def integrate_ref(self, depth, cam_view, tan_half_fov, colour=None, carve=True, z_min=0.05):
    """A stand-in for TsdfVolume.integrate on the CPU: the fp64 reference continued from, and rounded back into, ``self.acc``"""
    planes, _ = volume_ref(self, depth.float().cpu(), None if colour is None else colour.float().cpu(), cam_view.float().cpu(), tan_half_fov,
                           z_min=z_min, carve=carve, acc=self.acc.cpu())
    self.acc.copy_(planes.float())
    self.n_views += int(depth.shape[0])


@functools.lru_cache(maxsize=None)
def sphere_case(V, S, R, spheres="one", half=HALF, dist=1.6):
    """Analytic depth maps of SPHERE / TWO_SPHERES / a small sphere from ``_cams(V, dist)`` with a pattern colour, the volume's
    geometry and both evaluations of the definition.  Computed once, shared, never modified."""
    from tests.test_gs_gpu import _cams
    from videomv_amd.gs_mesh import TsdfVolume
    sp = {"one": SPHERE, "two": TWO_SPHERES, "small": [((0.05, -0.03, 0.02), 0.15)]}[spheres]
    cv, _ = _cams(V, dist=dist)
    depth = spheres_depth(cv, S, sp).float()
    colour = pattern_colour(V, S)
    vol = TsdfVolume(R, half, device="cpu")
    planes, margin = volume_ref(vol, depth, colour, cv)
    planes32, _ = volume_ref(vol, depth, colour, cv, dtype=torch.float32)
    return dict(V=V, S=S, R=R, half=half, spheres=sp, views=cv, depth=depth, colour=colour, voxel=vol.voxel, origin=vol.origin,
                planes=planes, margin=margin, planes32=planes32)


def field_of(planes, n_views, half, min_weight=1):
    """planes [7, R, R, R] -> a CPU TsdfVolume holding them (for .field / .colours / .extract)"""
    from videomv_amd.gs_mesh import TsdfVolume
    vol = TsdfVolume(int(planes.shape[-1]), half, device="cpu")
    vol.acc.copy_(planes.float())
    vol.n_views = n_views
    return vol


def check_sphere_mesh(verts, faces, case, max_dist, mean_dist, vol_lo, vol_hi, strict=True):
    """the analytic assertions on a mesh fused from a sphere case; prints every figure before it asserts -> the stats"""
    from videomv_amd.gs_mesh import mesh_stats
    st = mesh_stats(verts, faces)
    d = sphere_distance(verts.cpu(), case["spheres"]) / case["voxel"]
    rel = st["volume"] / sum(sphere_volume(r) for _, r in case["spheres"]) - 1.0
    print(f"mesh (V, S, R) = ({case['V']}, {case['S']}, {case['R']}): {st}, distance max {float(d.max()):.3f} mean {float(d.mean()):.3f} voxel, "
          f"volume {100 * rel:+.2f} %")
    if strict:
        assert st["euler"] == 2 and st["open_edges"] == 0 and st["misoriented"] == 0, st
    assert float(d.max()) <= max_dist and (mean_dist is None or float(d.mean()) <= mean_dist), (float(d.max()), float(d.mean()))
    assert vol_lo <= rel <= vol_hi, rel
    return st
