"""TSDF fusion on the device (csrc/gs_tsdf.hip through vmv_gs_tsdf_integrate and gs_mesh.TsdfVolume) against the fp64 restatement of
tests/gs_tsdf_ref.py (checked on the CPU in tests/test_gs_mesh_cpu.py), the shapes at which the kernel can go wrong, determinism and
accumulation, the store and read footprints, the mesh extracted on the device, and the entrance key gs_mesh.

The bound on the sums, per case: ten times the largest error of the same definition evaluated in fp32 on the CPU against fp64, over the
voxels no decision of which lies within 1e-4 of its threshold (the yardstick rule of tests/test_gs_ssim_gpu.py); the counts W, n_behind
and Wc of those voxels are exact.  Every test prints its figures before it asserts (DESIGN.md §5.4 quotes them)."""
import ctypes as C
import functools
import math
import os

import pytest
import torch

from tests import footprint as FP
from tests.gs_tsdf_ref import CLEAR, HALF, TAN, check_sphere_mesh, f32, field_of, sphere_case, volume_ref
from tests.test_gs_gpu import _cams, _scene

pytestmark = pytest.mark.gpu


def _volume(case, colour=True, device="cuda"):
    from videomv_amd.gs_mesh import TsdfVolume
    vol = TsdfVolume(case["R"], case["half"], device=device)
    vol.integrate(case["depth"], case["views"], TAN, colour=case["colour"] if colour else None)
    return vol


def _compare(name, acc, case):
    """counts exact and sums within 10 x the fp32 evaluation's own error, on the clear voxels; prints every figure before it asserts"""
    clear = case["margin"] >= CLEAR
    unclear = 1.0 - float(clear.double().mean())
    got, ref, ref32 = acc.detach().cpu().double(), case["planes"], case["planes32"].double()
    fig = {}
    for what, sl in (("tsdf", slice(0, 1)), ("rgb", slice(3, 6))):
        fig[what] = (float((got[sl] - ref[sl])[:, clear].abs().max()), 10.0 * float((ref32[sl] - ref[sl])[:, clear].abs().max()))
    wrong = {k: int((got[i] != ref[i])[clear].sum()) for k, i in (("W", 1), ("n_behind", 2), ("Wc", 6))}
    print(f"{name}: unclear {100 * unclear:.2f} %, sum tsdf error {fig['tsdf'][0]:.2e} (bound {fig['tsdf'][1]:.2e}), "
          f"sum RGB error {fig['rgb'][0]:.2e} (bound {fig['rgb'][1]:.2e}), wrong counts {wrong}, W > 0 on {int((ref[1] > 0).sum())}, "
          f"hidden somewhere {int((ref[2] > 0).sum())}, coloured {int((ref[6] > 0).sum())} of {clear.numel()}")
    assert unclear <= 0.01
    assert wrong == dict(W=0, n_behind=0, Wc=0)
    assert fig["tsdf"][0] <= fig["tsdf"][1] and fig["rgb"][0] <= fig["rgb"][1], fig
    assert int((ref[1] > 0).sum()) > 0 and int((ref[6] > 0).sum()) > 0          # the case reaches the fused and the coloured branch
    return fig


@functools.lru_cache(maxsize=None)
def _rendered_case():
    """real render output: _scene(300, 4) through render_depth at 64 px, 3 views, fused at R = 24; shared, never modified"""
    from videomv_amd.gs_export import _unpremultiplied
    from videomv_amd.gs import GaussianRenderer
    from videomv_amd.gs_mesh import TsdfVolume
    g = _scene(300, 4)
    cv, cvp = _cams(3)
    r = GaussianRenderer(output_size=64)
    out = r.render_depth(g.cuda().unsqueeze(0), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None, bg_color=torch.full((3,), 0.5).cuda())
    torch.cuda.synchronize()
    depth, colour = out["median_depth"][0, :, 0].cpu(), _unpremultiplied(out, 0.5).cpu()
    vol = TsdfVolume(24, 0.6, device="cpu")
    planes, margin = volume_ref(vol, depth, colour, cv)
    planes32, _ = volume_ref(vol, depth, colour, cv, dtype=torch.float32)
    return dict(V=3, S=64, R=24, half=0.6, views=cv, depth=depth, colour=colour, planes=planes, margin=margin, planes32=planes32)


CASES = {"sphere-6-48-16": (6, 48, 16), "sphere-12-96-32": (12, 96, 32), "two-spheres": (8, 64, 32, "two", 0.45),
         # x rows that are no multiple of the wave and a partial last block (17^3 = 19 x 256 + 49, 31^3 = 116 x 256 + 95, 33^3 = 140 x 256 + 97),
         # an image that is no multiple of anything, and a single view
         "R17-S40": (3, 40, 17), "R31-S40": (3, 40, 31), "R33-S40": (3, 40, 33), "one-view": (1, 48, 16)}


@pytest.mark.parametrize("name", list(CASES) + ["rendered"])
def test_kernel_matches_the_reference(name):
    case = _rendered_case() if name == "rendered" else sphere_case(*CASES[name])
    if name == "rendered":
        assert 0.02 < float((case["depth"] > 0).float().mean()) < 0.9 and bool((case["depth"] == 0).any())       # both kinds of pixel
    vol = _volume(case)
    torch.cuda.synchronize()
    assert vol.n_views == case["V"]
    _compare(name, vol.acc, case)


def test_camera_inside_the_cube():
    """two cameras 0.3 from the centre of a cube of half-width 0.542: voxels behind the camera plane and next to it (z <= z_min: skipped;
    just past it the pixel coordinate is enormous) — the range test on the float keeps them out, and the rest matches the reference"""
    case = sphere_case(2, 40, 17, "small", HALF, 0.3)
    i = torch.arange(17, dtype=torch.float64)
    z, y, x = torch.meshgrid(*(f32(case["origin"][k]) + i * f32(case["voxel"]) for k in (2, 1, 0)), indexing="ij")
    m = case["views"][0].double()
    zc = x * m[0, 2] + y * m[1, 2] + z * m[2, 2] + m[3, 2]
    px = ((x * m[0, 0] + y * m[1, 0] + z * m[2, 0] + m[3, 0]) / (zc * TAN) + 1) * 20
    assert int((zc <= 0.05).sum()) > 500 and int((zc > 0.05).sum()) > 500 and float(px[zc > 0.05].abs().max()) > 100
    vol = _volume(case)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vol.acc).all())
    _compare("camera inside", vol.acc, case)


def test_a_view_that_looks_away_changes_nothing():
    case = sphere_case(3, 40, 17)
    from videomv_amd.gs_mesh import TsdfVolume
    away = case["views"].clone()
    away[:, :, 2] = -away[:, :, 2]                                     # every voxel has z < 0
    vol = TsdfVolume(17, HALF, device="cuda")
    before = torch.rand(7, 17, 17, 17, generator=torch.Generator().manual_seed(3)) * 5
    vol.acc.copy_(before)
    vol.integrate(case["depth"], away, TAN, colour=case["colour"])
    torch.cuda.synchronize()
    assert torch.equal(vol.acc.cpu(), before)


def test_colour_null_leaves_its_planes_alone():
    case = sphere_case(3, 40, 17)
    from videomv_amd.gs_mesh import TsdfVolume
    with_colour = _volume(case)
    vol = TsdfVolume(17, HALF, device="cuda")
    before = torch.rand(4, 17, 17, 17, generator=torch.Generator().manual_seed(4))
    vol.acc[3:].copy_(before)
    vol.integrate(case["depth"], case["views"], TAN)
    torch.cuda.synchronize()
    assert torch.equal(vol.acc[3:].cpu(), before) and torch.equal(vol.acc[:3], with_colour.acc[:3]) and float(vol.acc[1].max()) == 3.0


def test_determinism_and_accumulation():
    """two calls give the same bits; views [0, k) then [k, V) give the bits of one call, for every k"""
    from videomv_amd.gs_mesh import TsdfVolume
    case = sphere_case(6, 48, 16)
    a, b = _volume(case), _volume(case)
    assert torch.equal(a.acc, b.acc)
    for k in (1, 3, 5):
        vol = TsdfVolume(16, HALF, device="cuda")
        vol.integrate(case["depth"][:k], case["views"][:k], TAN, colour=case["colour"][:k])
        vol.integrate(case["depth"][k:], case["views"][k:], TAN, colour=case["colour"][k:])
        assert vol.n_views == 6 and torch.equal(vol.acc, a.acc), k
    torch.cuda.synchronize()


def _raw(case, depth_ptr, colour_ptr, views_ptr, acc_ptr, stride):
    from videomv_amd import _lib as L
    from videomv_amd.gs_mesh import TsdfVolume
    from videomv_amd.ops import _stream_ptr
    geo = TsdfVolume(case["R"], case["half"], device="cpu")
    p = L.GsTsdfParams()
    p.depth, p.colour, p.views, p.n_views, p.size, p.tan_half_fov, p.res = depth_ptr, colour_ptr, views_ptr, case["V"], case["S"], TAN, case["R"]
    p.origin[0], p.origin[1], p.origin[2] = geo.origin
    p.voxel, p.trunc, p.z_min, p.carve, p.acc, p.plane_stride = geo.voxel, geo.trunc, 0.05, 1, acc_ptr, stride
    L.check(L.load().vmv_gs_tsdf_integrate(C.byref(p), _stream_ptr()), "gs_tsdf_integrate")


def test_store_and_read_footprint():
    """acc as 7 rows of a wider arena (plane_stride = R^3 + 37, the pointer 5 floats into the row): the guard floats between and around
    the planes are the bits they were; depth, colour and views with NaN all around them: the result is that of the plain call."""
    case = sphere_case(3, 40, 17)
    V, S, n = 3, 40, 17 ** 3
    acc = FP.Arena(7, n, kind="f32", ld=n + 37, col_off=5, g_after=8)
    ins = {"depth": FP.Arena(V * S, S, kind="f32", poison="nan", data=case["depth"].reshape(V * S, S), g_after=8),
           "colour": FP.Arena(V * 3 * S, S, kind="f32", poison="nan", data=case["colour"].reshape(V * 3 * S, S), g_after=8),
           "views": FP.Arena(V, 16, kind="f32", poison="nan", data=case["views"].reshape(V, 16), g_after=8)}
    buf = acc.buf.clone().cuda()
    bufs = {k: a.buf.clone().cuda() for k, a in ins.items()}
    assert acc.holds(0, 6 * (n + 37) + n) and all(bool(torch.isnan(b).any()) for b in bufs.values())
    _raw(case, ins["depth"].ptr(bufs["depth"]), ins["colour"].ptr(bufs["colour"]), ins["views"].ptr(bufs["views"]), acc.ptr(buf), n + 37)
    torch.cuda.synchronize()
    assert FP.stray_report("acc", acc, buf) == ""
    plain = _volume(case)
    assert torch.equal(acc.payload(buf), plain.acc.reshape(7, n)) and float(plain.acc[6].max()) > 0
    _compare("arena", acc.payload(buf).reshape(7, 17, 17, 17), case)


@pytest.mark.parametrize("V,S,R", [(6, 48, 16), (12, 96, 32)])
def test_mesh_from_device_accumulators(V, S, R):
    """extracted on the device from the kernel's planes: the CPU test's analytic assertions (not its counts), and the CPU's surface nets
    on the same planes give the same faces and, to 1e-6, the same vertices"""
    case = sphere_case(V, S, R)
    vol = _volume(case)
    verts, cols, faces = vol.extract()
    torch.cuda.synchronize()
    assert verts.is_cuda and faces.is_cuda and cols.is_cuda
    check_sphere_mesh(verts, faces, case, 1.5, 0.25, -0.10, 0.02)
    f, valid = vol.field()
    assert int(((vol.acc[1] == 0) & valid).sum()) > 0                  # solid by the every-view rule
    v_cpu, c_cpu, f_cpu = field_of(vol.acc.cpu(), V, HALF).extract()
    assert torch.equal(faces.cpu(), f_cpu)
    assert float((verts.cpu() - v_cpu).abs().max()) <= 1e-6 and float((cols.cpu() - c_cpu).abs().max()) <= 1e-6


def test_t2v_entrance_exports_a_mesh(tmp_path):
    """Two prompts with 8 orbit views and gs_mesh at 32^3: a mesh file per prompt, finite, inside the fusion cube; every other output is
    that of the run without the key.  With the default cube (half-width 2 sin 19.8 deg = 0.677 about the origin) the RANDOM-weight
    model of this test gives a mesh without faces: its Gaussians fill the LGM's whole position range [-1, 1]^3, the first orbit camera
    sees them as a wall at depth 1.0 .. 1.4, in front of the cube (depth 1.32 and more), and the other seven look past the cube
    (measured on the CPU interpreter: the share of pixels with a median depth is 1, 0, 0, 0, 0, 0, 0, 0 per view; 183 of 32 768 voxels
    fused, no cell with eight valid corners and a sign change).  So the mesh with faces is asked of a third run whose cube,
    gs_mesh_extent 1.2, holds that range."""
    from tests.test_gs_depth_gpu import _entrance_cfg
    from videomv_amd.gs_mesh import load_mesh_ply
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    base = ["save_gaussians", "True", "gs_orbit_views", "8"]
    mesh = base + ["gs_mesh", "True", "gs_mesh_res", "32"]
    runs = {}
    for name, extra in (("plain", base), ("mesh", mesh), ("wide", mesh + ["gs_mesh_extent", "1.2"])):
        cu = _entrance_cfg(tmp_path / name, extra)
        runs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    files = {k: sorted(os.path.relpath(os.path.join(d, f), r.log_dir) for d, _, fs in os.walk(r.log_dir) for f in fs) for k, r in runs.items()}
    for name, half in (("mesh", 2.0 * math.sin(math.radians(39.6 / 2))), ("wide", 1.2)):       # default: the t2v orbit's distance x sin(fovy / 2)
        cfg = runs[name]
        assert len(cfg.gs_exports) == 2
        for e in cfg.gs_exports:
            verts, rgb, faces = load_mesh_ply(e["mesh_ply"])
            print(name, e["mesh_ply"], e["mesh_vertices"], e["mesh_faces"], e["mesh_open_edges"])
            assert verts.shape == rgb.shape == (e["mesh_vertices"], 3) and faces.shape == (e["mesh_faces"], 3)
            assert torch.isfinite(verts).all() and (verts.shape[0] == 0 or float(verts.abs().max()) <= half)
            if name == "wide":
                assert e["mesh_faces"] > 0 and int(faces.max()) < verts.shape[0] and int(faces.min()) >= 0
        assert [f for f in files[name] if not f.endswith("_gs_mesh.ply")] == files["plain"] and len(files[name]) == len(files["plain"]) + 2
        for f in files["plain"]:
            a, b = (os.path.join(runs[k].log_dir, f) for k in ("plain", name))
            if f.endswith(".pt"):
                assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"]), f
            elif f.endswith((".ply", ".png")):
                assert open(a, "rb").read() == open(b, "rb").read(), f
