"""The mesh export without a GPU: the ABI of vmv_gs_tsdf_integrate, surface nets on analytic fields, the fp64 restatement of the fusion
(tests/gs_tsdf_ref.py) carried through ``TsdfVolume.field`` and ``surface_nets`` to meshes of spheres with analytic bounds, the .ply
writer, and the entrance keys gs_mesh / gs_mesh_* on the CPU plan interpreter.  The GPU tests (tests/test_gs_mesh_gpu.py) hold the
kernel to the same reference and the device's meshes to the same bounds."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

from tests import plan_interp
from tests.gs_tsdf_ref import (CLEAR, HALF, SPHERE, TAN, TWO_SPHERES, check_sphere_mesh, field_of, integrate_ref, pattern_colour, sphere_case,
                               sphere_depth, sphere_distance, sphere_volume, spheres_depth, volume_ref)
from tests.test_gs_depth_cpu import _install_render_depth
from tests.test_gs_export_cpu import _files, _tiny_cfg
from tests.test_gs_gpu import _cams
from videomv_amd.gs_mesh import TsdfVolume, load_mesh_ply, mesh_stats, save_mesh_ply, surface_nets


# ------------------------------------------------------------------------------------------------------------------------ ABI
def _params(**kw):
    from videomv_amd import _lib as L
    keep = torch.zeros(16 * 16 + 16 + 7 * 8 + 8)
    p = L.GsTsdfParams()
    p.depth = p.views = p.acc = keep.data_ptr()
    p.n_views, p.size, p.tan_half_fov, p.res = 1, 16, 0.36, 2
    p.voxel, p.trunc, p.z_min, p.carve, p.plane_stride = 0.1, 0.3, 0.05, 1, 8
    for k, v in kw.items():
        setattr(p, k, v)
    return p, keep


def test_tsdf_params_abi_and_validation_without_a_device():
    """every refusal of the header's list, none of which may touch a device (there is none here); a valid block is not tried: it would launch"""
    from videomv_amd import _lib as L
    lib = L.load()
    assert lib.vmv_abi_version() == L.ABI_VERSION == 12
    assert lib.vmv_sizeof(109) == C.sizeof(L.GsTsdfParams) == 88
    assert L.GsTsdfParams.origin.offset == 40 and L.GsTsdfParams.acc.offset == 72 and L.GsTsdfParams.plane_stride.offset == 80
    assert "vmv_gs_tsdf_integrate" in L.SYMBOLS
    call = lambda p: lib.vmv_gs_tsdf_integrate(C.byref(p[0]), None)
    assert lib.vmv_gs_tsdf_integrate(None, None) == -3
    for field in ("depth", "views", "acc"):
        assert call(_params(**{field: None})) == -3, field
    for bad in (dict(n_views=0), dict(size=0), dict(res=1), dict(res=1025, plane_stride=1025 ** 3), dict(tan_half_fov=0.0), dict(voxel=0.0),
                dict(voxel=-0.1), dict(trunc=0.0), dict(z_min=0.0), dict(z_min=float("nan")), dict(plane_stride=7), dict(res=3)):
        assert call(_params(**bad)) == -1, bad
    assert call(_params(size=32769)) == -4                              # VMV_ERANGE: the kernel's 32-bit pixel offsets
    base = _params()[1].data_ptr()
    for field in ("depth", "colour", "views", "acc"):
        p = _params()
        setattr(p[0], field, p[1].data_ptr() + 2)
        assert call(p) == -2, field
    assert base % 4 == 0


# ------------------------------------------------------------------------------------------------- surface nets on analytic fields
def _grid(R, half):
    voxel = 2.0 * half / R
    o = -half + 0.5 * voxel
    i = o + torch.arange(R, dtype=torch.float64) * voxel
    z, y, x = torch.meshgrid(i, i, i, indexing="ij")
    return x, y, z, voxel, (o, o, o)


def _analytic(sd, voxel):
    f = (sd / (3.0 * voxel)).clamp(-1, 1).float()
    return f, torch.ones_like(f, dtype=torch.bool)


def test_surface_nets_sphere():
    """off-centre sphere r = 0.5 in a cube of half-width 0.8 at R = 24: closed, oriented, genus 0; vertices on the sphere to a quarter
    voxel; the volume of the inscribed polyhedron 5 % at the most below the sphere's (measured: 0.048 voxel, -2.0 %)"""
    c, r = (0.07, -0.05, 0.11), 0.5
    x, y, z, voxel, o = _grid(24, 0.8)
    f, valid = _analytic(((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2).sqrt() - r, voxel)
    colour = torch.stack([x, y, z]).float() * 0.5 + 0.5
    verts, cols, faces = surface_nets(f, valid, o, voxel, colour=colour)
    st = mesh_stats(verts, faces)
    d = sphere_distance(verts, [(c, r)]) / voxel
    rel = st["volume"] / sphere_volume(r) - 1.0
    print(st, f"distance max {float(d.max()):.3f} voxel, volume {100 * rel:+.2f} %")
    assert st["euler"] == 2 and st["open_edges"] == 0 and st["misoriented"] == 0 and st["vertices"] == verts.shape[0] > 500
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64 and cols.shape == verts.shape
    assert float(d.max()) <= 0.25 and abs(rel) <= 0.05 and st["volume"] > 0
    # the colour field is linear in position: the mean of a cell's 8 corners is the colour of the cell's centre, within a voxel of the vertex
    assert float((cols - (verts * 0.5 + 0.5)).abs().max()) <= 0.5 * voxel + 1e-6
    # deterministic: the same call gives the same tensors
    again = surface_nets(f, valid, o, voxel, colour=colour)
    assert all(torch.equal(a, b) for a, b in zip((verts, cols, faces), again))


def test_surface_nets_torus():
    x, y, z, voxel, o = _grid(32, 0.8)
    f, valid = _analytic((((x * x + y * y).sqrt() - 0.45) ** 2 + z * z).sqrt() - 0.18, voxel)
    verts, _, faces = surface_nets(f, valid, o, voxel)
    st = mesh_stats(verts, faces)
    print(st)
    assert st["euler"] == 0 and st["open_edges"] == 0 and st["misoriented"] == 0 and st["faces"] == 2 * st["vertices"]
    assert st["volume"] == pytest.approx(2 * math.pi ** 2 * 0.45 * 0.18 ** 2, rel=0.05)


def test_surface_nets_skips_cells_with_an_invalid_corner():
    c, r = (0.0, 0.0, 0.0), 0.5
    x, y, z, voxel, o = _grid(24, 0.8)
    f, valid = _analytic((x * x + y * y + z * z).sqrt() - r, voxel)
    octant = (x > 0) & (y > 0) & (z > 0)
    verts, _, faces = surface_nets(f, valid & ~octant, o, voxel)
    st = mesh_stats(verts, faces)
    assert st["faces"] > 0 and st["open_edges"] > 0 and st["misoriented"] == 0
    # a cell that touches the octant has a corner in it: no vertex beyond the first voxel centres outside it
    lo = o[0] + 12 * voxel                                             # the octant's first voxel centre
    assert not bool(((verts > lo - voxel + 1e-6).all(dim=1)).any())
    full = mesh_stats(*surface_nets(f, valid, o, voxel)[::2])
    assert full["open_edges"] == 0 and full["faces"] > st["faces"]
    # nothing crosses zero / nothing is valid: an empty mesh, not an error
    for ff, vv in ((f.abs() + 0.1, valid), (f, torch.zeros_like(valid))):
        v0, c0, f0 = surface_nets(ff, vv, o, voxel)
        assert v0.shape == (0, 3) and c0.shape == (0, 3) and f0.shape == (0, 3) and f0.dtype == torch.int64


# ----------------------------------------------------------------------------------------------------------- fusion, then mesh
@pytest.mark.parametrize("V,S,R,solid", [(6, 48, 16, 57), (12, 96, 32, 1635)])
def test_fused_sphere_is_a_closed_sphere(V, S, R, solid):
    """sphere r = 0.32 seen by V cameras at elevation 15 deg, fused by the fp64 reference: the mesh is closed and oriented, every vertex
    within 1.5 voxels of the sphere (the caps, which the one-elevation orbit sees at grazing angles only, come from the visual hull:
    measured 0.37 / 0.78), 0.25 on average (0.11), the volume -10 % .. +2 % (-7.8 % / -3.1 %); some voxels are solid only by the
    "hidden in every view" rule; at most 1 % of the voxels sit within 1e-4 of a decision."""
    case = sphere_case(V, S, R)
    vol = field_of(case["planes"], V, HALF)
    f, valid = vol.field()
    n_solid = int(((vol.acc[1] == 0) & valid).sum())
    unclear = float((case["margin"] < CLEAR).double().mean())
    err32 = float((case["planes32"].double() - case["planes"])[:, case["margin"] >= CLEAR].abs().max())
    print(f"solid by the every-view rule {n_solid}, unclear {100 * unclear:.2f} %, fp32 error of the sums {err32:.2e}")
    assert n_solid == solid and bool((f[(vol.acc[1] == 0) & valid] == -1).all())
    assert unclear <= 0.01
    verts, cols, faces = vol.extract()
    check_sphere_mesh(verts, faces, case, 1.5, 0.25, -0.10, 0.02)
    assert float(cols.min()) >= 0.0 and float(cols.max()) <= 1.0


def test_hidden_in_any_view_would_not_be_the_rule():
    """voxels hidden in some but not all views, never fused: invalid, not solid"""
    case = sphere_case(6, 48, 16)
    vol = field_of(case["planes"], 6, HALF)
    f, valid = vol.field()
    some = (vol.acc[1] == 0) & (vol.acc[2] > 0) & (vol.acc[2] < 6)
    assert not bool(valid[some].any()) and bool((f[~valid] == 0).all())
    assert not bool(field_of(case["planes"], 7, HALF).field()[1][vol.acc[1] == 0].any())      # one more view integrated that saw none of them


def test_two_spheres_do_not_shadow_each_other():
    """a sheet in the shadow one sphere casts on the other would put vertices far from both (measured max 0.45 voxel, volume -7.4 %)"""
    case = sphere_case(8, 64, 32, "two", 0.45)
    vol = field_of(case["planes"], 8, 0.45)
    verts, _, faces = vol.extract()
    st = check_sphere_mesh(verts, faces, case, 1.0, None, -0.15, 0.15, strict=False)
    assert st["faces"] > 500 and float((case["margin"] < CLEAR).double().mean()) <= 0.01


def test_carve_off_leaves_background_voxels_unobserved():
    case = sphere_case(6, 48, 16)
    vol = TsdfVolume(16, HALF, device="cpu")
    planes, _ = volume_ref(vol, case["depth"], None, case["views"], carve=False)
    carved = case["planes"]
    only_background = (carved[1] > 0) & (planes[1] == 0)
    assert int(only_background.sum()) > 100 and bool((planes[0][only_background] == 0).all())
    assert bool((carved[0][only_background] == carved[1][only_background]).all())        # carved: tsdf = 1 per view that saw them
    assert torch.equal(planes[2], carved[2]) and bool((planes[3:] == 0).all())             # no colour given: planes 3..6 stay zero


def test_constant_view_colours_give_their_mean():
    case = sphere_case(6, 48, 16)
    V, S = 6, 48
    per_view = torch.tensor([[0.1 * v, 1.0 - 0.1 * v, 0.5 + 0.05 * v] for v in range(V)], dtype=torch.float64)
    colour = per_view.float().view(V, 3, 1, 1).expand(V, 3, S, S).contiguous()
    vol = TsdfVolume(16, HALF, device="cpu")
    planes, _ = volume_ref(vol, case["depth"], colour, case["views"])
    counted = torch.stack([volume_ref(vol, case["depth"][v:v + 1], colour[v:v + 1], case["views"][v:v + 1])[0][6] for v in range(V)])
    assert torch.equal(counted.sum(0), planes[6]) and int((planes[6] > 1).sum()) > 50
    want = torch.einsum("vzyx,vc->czyx", counted, per_view.float().double()) / planes[6].clamp_min(1)
    got = field_of(planes, V, HALF).colours().double()
    seen = planes[6] > 0
    assert float((got - want)[:, seen].abs().max()) < 1e-6 and bool((got[:, ~seen] == 0.5).all())


def test_field_and_colours_on_hand_made_planes():
    vol = TsdfVolume(2, 1.0, centre=(1.0, 2.0, 3.0), device="cpu")
    assert vol.voxel == 1.0 and vol.origin == (0.5, 1.5, 2.5) and vol.trunc == 3.0 and vol.acc.shape == (7, 2, 2, 2) and vol.n_views == 0
    assert TsdfVolume(4, 1.0, trunc=0.2, device="cpu").trunc == 0.2
    a = vol.acc.view(7, 8)
    #              fused      fused x3   hidden in all  hidden in some   never seen   weight below min
    a[0, :6] = torch.tensor([0.5, -1.5, 0.0, 0.0, 0.0, 0.25])
    a[1, :6] = torch.tensor([1.0, 3.0, 0.0, 0.0, 0.0, 1.0])
    a[2, :6] = torch.tensor([0.0, 1.0, 4.0, 3.0, 0.0, 0.0])
    a[3:6, 0] = torch.tensor([0.2, 0.4, 0.6])
    a[3:6, 1] = torch.tensor([0.6, 1.2, 1.8])
    a[6, :2] = torch.tensor([1.0, 2.0])
    vol.n_views = 4
    f, valid = vol.field()
    assert f.view(8)[:6].tolist() == [0.5, -0.5, -1.0, 0.0, 0.0, 0.25] and valid.view(8)[:6].tolist() == [True, True, True, False, False, True]
    f2, valid2 = vol.field(min_weight=2)
    assert valid2.view(8)[:6].tolist() == [False, True, True, False, False, False] and f2.view(8)[:3].tolist() == [0.0, -0.5, -1.0]
    col = vol.colours().view(3, 8)
    assert torch.allclose(col[:, 0], torch.tensor([0.2, 0.4, 0.6])) and torch.allclose(col[:, 1], torch.tensor([0.3, 0.6, 0.9]))
    assert bool((col[:, 2:] == 0.5).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate(torch.zeros(1, 4, 4), torch.eye(4).unsqueeze(0), TAN)


def test_sphere_depth_is_the_depth_of_points_on_the_sphere():
    """the analytic depth, unprojected with the renderer's own convention, lies on the sphere; the silhouette is a disc of the right size"""
    from videomv_amd.gs import depth_to_points
    cv, _ = _cams(3)
    (c, r), = SPHERE
    for v in range(3):
        d = sphere_depth(cv[v], 64, c, r)
        pts, _ = depth_to_points(d.float(), cv[v], TAN)
        assert pts.shape[0] > 300 and float(sphere_distance(pts, SPHERE).max()) < 1e-5
    both = spheres_depth(cv, 64, TWO_SPHERES)
    singles = [spheres_depth(cv, 64, [s]) for s in TWO_SPHERES]
    assert torch.equal(both > 0, (singles[0] > 0) | (singles[1] > 0))
    overlap = (singles[0] > 0) & (singles[1] > 0)
    assert torch.equal(both[overlap], torch.minimum(singles[0], singles[1])[overlap])


# ------------------------------------------------------------------------------------------------------------------------ .ply
def test_mesh_ply_round_trip(tmp_path):
    gen = torch.Generator().manual_seed(7)
    verts, cols = torch.randn(11, 3, generator=gen), torch.rand(11, 3, generator=gen)
    faces = torch.randint(0, 11, (17, 3), generator=gen)
    path = str(tmp_path / "m.ply")
    assert save_mesh_ply(verts, cols, faces, path) == (11, 17)
    with open(path, "rb") as fh:
        data = fh.read()
    head, body = data.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n")[:-1] == ["ply", "format binary_little_endian 1.0", "element vertex 11", "property float x",
                                                     "property float y", "property float z", "property uchar red", "property uchar green",
                                                     "property uchar blue", "element face 17", "property list uchar int vertex_indices"]
    assert len(body) == 11 * 15 + 17 * 13
    vrows = [struct.unpack("<3f3B", body[15 * i:15 * (i + 1)]) for i in range(11)]                  # an independent reader
    frows = [struct.unpack("<B3i", body[165 + 13 * i:165 + 13 * (i + 1)]) for i in range(17)]
    assert np.array_equal(np.array([r[:3] for r in vrows], dtype=np.float32), verts.numpy())
    assert np.array_equal(np.array([r[3:] for r in vrows]), np.floor(cols.numpy() * 255.0 + 0.5).astype(np.int64))
    assert all(r[0] == 3 for r in frows) and np.array_equal(np.array([r[1:] for r in frows]), faces.numpy())
    v, rgb, f = load_mesh_ply(path)
    assert torch.equal(v, verts) and torch.equal(f, faces) and f.dtype == torch.int64 and rgb.dtype == torch.uint8
    assert float((rgb.float() / 255 - cols).abs().max()) <= 0.5 / 255 + 1e-6
    assert save_mesh_ply(verts, cols, faces[:0], path) == (11, 0)
    v, rgb, f = load_mesh_ply(path)
    assert torch.equal(v, verts) and f.shape == (0, 3)
    assert save_mesh_ply(verts[:0], cols[:0], faces[:0], path) == (0, 0) and load_mesh_ply(path)[0].shape == (0, 3)
    from videomv_amd.gs import save_points_ply
    save_points_ply(verts, cols, path)
    with pytest.raises(ValueError, match="save_mesh_ply"):
        load_mesh_ply(path)


def test_mesh_stats_on_a_tetrahedron():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])                                  # outward
    st = mesh_stats(v, f)
    assert st == dict(vertices=4, edges=6, faces=4, euler=2, open_edges=0, misoriented=0, volume=pytest.approx(1 / 6))
    flipped = f.clone()
    flipped[3] = torch.tensor([1, 3, 2])
    st = mesh_stats(v, flipped)
    assert st["misoriented"] == 3 and st["open_edges"] == 0
    st = mesh_stats(v, f[:3])
    assert st["open_edges"] == 3 and st["euler"] == 1 and st["misoriented"] == 0


# ------------------------------------------------------------------------------------------------------------------- entrance
MESH = ["gs_orbit_views", "3", "gs_orbit_size", "32", "gs_mesh", "True", "gs_mesh_res", "16"]


@pytest.mark.parametrize("extra", [["gs_mesh", "True", "gs_orbit_views", "3"], ["save_gaussians", "True", "gs_mesh", "True"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh_res", "64"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh_extent", "0.5"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh_trunc", "0.05"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh", "True", "gs_mesh_res", "8"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh", "True", "gs_mesh_res", "1024"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh", "True", "gs_mesh_extent", "-0.5"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh", "True", "gs_mesh_extent", "0"],
                                   ["save_gaussians", "True", "gs_orbit_views", "3", "gs_mesh", "True", "gs_mesh_trunc", "-1"]])
def test_mesh_keys_are_refused_before_sampling(monkeypatch, tmp_path, extra):
    """gs_mesh without save_gaussians or without orbit views, a sub-key without gs_mesh, a resolution outside [16, 512], an extent or a
    truncation that is not positive: refused, nothing sampled, nothing written"""
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, extra)
    with pytest.raises(Exception, match="gs_mesh"):
        INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    assert not os.path.exists(tmp_path / "out")


def test_entrance_writes_a_mesh_and_nothing_else_changes(monkeypatch, tmp_path):
    """save_gaussians with 3 orbit views of 32 px and gs_mesh at 16^3: the orbit is rendered ONCE (render_depth, no render), one fusion
    call sees its 3 median-depth maps and colours in [0, 1], the mesh loads and ``rec`` carries its counts; every other file and the
    latents are those of the run without the key."""
    plan_interp.install(monkeypatch)
    calls = _install_render_depth(monkeypatch)
    from videomv_amd import gs as _gs
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    fused = []

    def integrate(self, depth, cam_view, tan_half_fov, colour=None, **kw):
        fused.append((tuple(depth.shape), tuple(cam_view.shape), tuple(colour.shape), float(colour.min()), float(colour.max()), self.res, self.voxel))
        integrate_ref(self, depth, cam_view, tan_half_fov, colour=colour, **kw)
    monkeypatch.setattr(TsdfVolume, "integrate", integrate)
    plain_render = _gs.GaussianRenderer.render
    renders = []
    monkeypatch.setattr(_gs.GaussianRenderer, "render", lambda self, *a, **k: (renders.append(1), plain_render(self, *a, **k))[1])
    base = ["save_gaussians", "True", "gs_fit_iters", "0", "gs_orbit_views", "3", "gs_orbit_size", "32"]
    cfgs = {}
    for name, extra in (("plain", base), ("mesh", base[:4] + MESH)):
        cu = _tiny_cfg(tmp_path / name, extra)
        n0 = len(renders)
        cfgs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
        assert len(renders) - n0 == (1 if name == "plain" else 0)
    assert calls == [(1, 3)] and len(fused) == 1
    d_shape, v_shape, c_shape, c_min, c_max, res, voxel = fused[0]
    assert d_shape == (3, 32, 32) and v_shape == (3, 4, 4) and c_shape == (3, 3, 32, 32) and 0.0 <= c_min <= c_max <= 1.0 and res == 16
    plain, mesh = (_files(cfgs[k].log_dir) for k in ("plain", "mesh"))
    new = [f for f in mesh if f.endswith("_gs_mesh.ply")]
    assert len(new) == 1 and [f for f in mesh if f not in new] == plain
    rec, = cfgs["mesh"].gs_exports
    rec0, = cfgs["plain"].gs_exports
    assert not any(k.startswith("mesh") for k in rec0)
    verts, rgb, faces = load_mesh_ply(rec["mesh_ply"])
    assert rec["mesh_vertices"] == verts.shape[0] and rec["mesh_faces"] == faces.shape[0] and torch.isfinite(verts).all()
    assert rec["mesh_open_edges"] == mesh_stats(verts, faces)["open_edges"]
    half = 0.5 * 16 * voxel                                            # the default cube: the t2v orbit's distance 2.0 x sin(39.6 deg / 2)
    assert half == pytest.approx(2.0 * math.sin(math.radians(39.6 / 2)), rel=1e-5) and (faces.shape[0] == 0 or float(verts.abs().max()) <= half)
    from PIL import Image
    for f in plain:
        a, b = (os.path.join(cfgs[k].log_dir, f) for k in ("plain", "mesh"))
        if f.endswith(".pt"):
            assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"])
        elif f.endswith(".png") and "_gs_orbit" in f:
            assert np.abs(np.array(Image.open(a)).astype(int) - np.array(Image.open(b)).astype(int)).max() <= 1      # oracle vs fp64 reference
        elif f.endswith(".ply"):
            assert open(a, "rb").read() == open(b, "rb").read()
