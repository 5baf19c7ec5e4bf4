"""Texture baking on the device (csrc/gs_mesh_bake.hip through vmv_gs_mesh_bake and gs_mesh.bake_texture) against the fp64 restatement of
tests/mesh_bake_ref.py (checked on the CPU in tests/test_gs_mesh_bake_cpu.py): the shapes at which the kernel can go wrong, determinism,
the store and read footprints, out-of-range indices, and the entrance key gs_mesh_texture.

The bound, per case: ten times the largest error of the same definition evaluated in fp32 on the CPU against fp64, over the texels no
decision of which lies within 1e-4 of its threshold; on those texels the sets {W > 0}, {W == 0} and {W == -1} are exact.  Every raw call
writes into four planes of a wider arena (plane_stride = T^2 + 37, the pointer 5 floats into the row) and a guarded status word: a store
outside the planes shows as a changed guard, not as a fault.  Every test prints its figures before it asserts."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import footprint as FP
from tests import mesh_bake_ref as B
from tests.gs_tsdf_ref import TAN, f32
from tests.test_gs_gpu import _cams, _scene
from tests.test_gs_mesh_bake_cpu import CASES, bake

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0x5A5A5A5A


def _raw(case, verts=None, cols=None, faces=None, depth=None, colour=None, views=None, stride=3, offset=0):
    """one call of vmv_gs_mesh_bake on the current stream.  ``verts`` / ``cols`` / ``depth`` / ``colour``: (arena, device buffer) pairs, dense
    tensors, or None for the case's own; ``faces``: an int64 device buffer read at ``offset`` + f * ``stride``; ``views``: a [V, 4, 4] tensor
    (depth and colour then have V views).  -> (planes [4, T, T] on the host, status, guards intact)"""
    from videomv_amd import _lib as L
    from videomv_amd.ops import _stream_ptr
    m, n, P = int(case["faces"].shape[0]), int(case["verts"].shape[0]), case["P"]
    T = case["ref"]["T"]
    keep = []

    def ptr(given, own):
        if isinstance(given, tuple):
            return given[0].ptr(given[1])
        keep.append((own if given is None else given).float().contiguous().cuda())
        return keep[-1].data_ptr()
    views = (case["views"] if views is None else views).float().contiguous().cuda()
    V, S = int(views.shape[0]), case["S"]
    faces_buf = case["faces"].reshape(-1).cuda() if faces is None else faces
    assert faces_buf.dtype == torch.int64 and faces_buf.is_cuda and faces_buf.is_contiguous()
    assert offset + (m - 1) * stride + 3 <= faces_buf.numel()          # bounds of the reads and stores, checked before the launch
    assert all(t is None or isinstance(t, tuple) or t.shape[0] == V for t in (depth, colour))
    out = FP.Arena(4, T * T, kind="f32", ld=T * T + 37, col_off=5, g_after=8)
    assert out.holds(0, 3 * (T * T + 37) + T * T)
    buf = out.buf.clone().cuda()
    status = torch.full((2 * GUARD + 1,), PATTERN, dtype=torch.int32, device="cuda")
    p = L.GsMeshBakeParams()
    p.verts, p.vert_colours = ptr(verts, case["verts"]), ptr(cols, case["cols"])
    p.faces, p.face_stride, p.n_faces, p.n_vertices = faces_buf.data_ptr() + 8 * offset, stride, m, n
    p.depth, p.colour, p.views = ptr(depth, case["depth"]), ptr(colour, case["colour"]), views.data_ptr()
    p.n_views, p.size, p.tan_half_fov, p.z_min, p.depth_tol, p.cos_min = V, S, TAN, 0.05, case["tol"], 0.1
    p.patch, p.tex_size, p.out, p.plane_stride, p.status = P, T, out.ptr(buf), T * T + 37, status.data_ptr() + 4 * GUARD
    L.check(L.load().vmv_gs_mesh_bake(C.byref(p), _stream_ptr()), "gs_mesh_bake")
    torch.cuda.synchronize()
    st = status.cpu()
    intact = FP.stray_report("out", out, buf) == "" and bool((st[:GUARD] == PATTERN).all()) and bool((st[GUARD + 1:] == PATTERN).all())
    return out.payload(buf).cpu().reshape(4, T, T), int(st[GUARD]), intact


@functools.lru_cache(maxsize=None)
def _rendered_case():
    """real render output: _scene(300, 4) through render_depth at 64 px, 3 views, fused at R = 24 over the cube of half-width 0.6 and
    extracted on the device; baked at patch 8 with a tolerance of 2 voxels; shared, never modified"""
    from videomv_amd.gs_export import _unpremultiplied
    from videomv_amd.gs import GaussianRenderer
    from videomv_amd.gs_mesh import TsdfVolume
    g = _scene(300, 4)
    cv, cvp = _cams(3)
    r = GaussianRenderer(output_size=64)
    out = r.render_depth(g.cuda().unsqueeze(0), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None, bg_color=torch.full((3,), 0.5).cuda())
    depth, colour = out["median_depth"][0, :, 0], _unpremultiplied(out, 0.5)
    vol = TsdfVolume(24, 0.6, device="cuda")
    vol.integrate(depth, cv, TAN, colour=colour)
    verts, cols, faces = vol.extract()
    torch.cuda.synchronize()
    return B._case(dict(V=3, S=64, R=24, P=8, views=cv, depth=depth.cpu(), colour=colour.cpu(), verts=verts.cpu(), cols=cols.cpu(),
                        faces=faces.cpu().contiguous(), tol=B.depth_tol_of(24, 0.6)))


def _get(name):
    return _rendered_case() if name == "rendered" else B.sphere_bake_case(*CASES[name])


@pytest.mark.parametrize("name", list(CASES) + ["rendered"])
def test_kernel_matches_the_reference(name):
    case = _get(name)
    m, P = case["faces"].shape[0], case["P"]
    if name == "rendered":
        assert m > 100 and 0.02 < float((case["depth"] > 0).float().mean()) < 0.9
    planes, status, intact = _raw(case)
    assert status == 0 and intact
    B.compare(name, planes, case)
    # the host layer gives the same bits, on the device, and counts what it wrote
    tex, uv, info = bake(case, device="cuda")
    assert tex.is_cuda and torch.equal(tex.cpu(), planes)
    assert info["size"] == case["ref"]["T"] and info["texels"] == (m // 2) * P * P + (m % 2) * (P * (P + 1) // 2)
    assert info["baked"] == int((planes[3] > 0).sum()) / info["texels"]


def test_a_view_that_looks_away_gives_the_bits_of_the_run_without_it():
    case = B.sphere_bake_case(3, 48, 16, 4)
    away = case["views"][:1].clone()
    away[:, :, 2] = -away[:, :, 2]                                     # every point has z < 0
    plain, status, intact = _raw(case)
    assert status == 0 and intact and int((plain[3] > 0).sum()) > 0
    for at in (0, 1, 3):                                                # first, in the middle, last
        order = list(range(at)) + [0] + list(range(at, 3))
        views = torch.cat([case["views"][:at], away, case["views"][at:]])
        got, status, intact = _raw(case, depth=case["depth"][order], colour=case["colour"][order], views=views)
        assert status == 0 and intact and torch.equal(got, plain), at


def test_two_calls_give_the_same_bits():
    for name in ("sphere-6-96-24-P8", "one-view-odd-patch"):
        case = _get(name)
        a, b = _raw(case), _raw(case)
        assert a[1] == b[1] == 0 and a[2] and b[2] and torch.equal(a[0], b[0]), name


def test_store_and_read_footprint():
    """the planes inside a wider arena (every raw call: guards intact); verts, vert_colours, depth and colour with NaN all around them and
    the faces at stride 5, 7 elements into a buffer whose gaps hold 2^62: the bits of the dense call, status 0 (a read of a gap would flag
    an index out of range, a read of a guard would put a NaN into a texel)"""
    case = B.sphere_bake_case(1, 40, 17, 5)
    V, S, n, m = 1, 40, case["verts"].shape[0], case["faces"].shape[0]
    plain, status, intact = _raw(case)
    assert status == 0 and intact and bool(torch.isfinite(plain).all())
    ins = {"verts": FP.Arena(n, 3, kind="f32", poison="nan", data=case["verts"], g_after=8),
           "cols": FP.Arena(n, 3, kind="f32", poison="nan", data=case["cols"], g_after=8),
           "depth": FP.Arena(V * S, S, kind="f32", poison="nan", data=case["depth"].reshape(V * S, S), g_after=8),
           "colour": FP.Arena(V * 3 * S, S, kind="f32", poison="nan", data=case["colour"].reshape(V * 3 * S, S), g_after=8)}
    bufs = {k: a.buf.clone().cuda() for k, a in ins.items()}
    assert all(bool(torch.isnan(b).any()) for b in bufs.values())
    wide = torch.full((7 + 5 * m + 9,), 2 ** 62, dtype=torch.int64)
    wide[7:7 + 5 * m].view(m, 5)[:, :3] = case["faces"]
    got, status, intact = _raw(case, faces=wide.cuda(), stride=5, offset=7, **{k: (ins[k], bufs[k]) for k in ins})
    assert status == 0 and intact and torch.equal(got, plain)
    for k, a in ins.items():                                            # and no input was written
        assert torch.equal(bufs[k].cpu().view(a.itype), a.buf.view(a.itype)), k
    # the host layer passes a strided view through as it is
    from videomv_amd.gs_mesh import bake_texture
    tex = bake_texture(case["verts"].cuda(), case["cols"].cuda(), wide[7:7 + 5 * m].view(m, 5).cuda()[:, :3], case["depth"].cuda(), case["colour"].cuda(),
                       case["views"].cuda(), f32(TAN), patch=5, depth_tol=case["tol"], cos_min=f32(0.1), z_min=f32(0.05))[0]
    assert torch.equal(tex.cpu(), plain)


def test_out_of_range_indices_are_flagged_and_their_faces_left_empty():
    """-1, -8, n and n + 8 in four faces: status bit 0, those faces' texels are those of no face, every other texel is the bits of the
    clean run, guards intact; bake_texture raises"""
    from videomv_amd.gs_mesh import bake_texture
    case = B.sphere_bake_case(3, 48, 16, 4)
    n, m = case["verts"].shape[0], case["faces"].shape[0]
    plain, status, intact = _raw(case)
    assert status == 0 and intact
    faces = case["faces"].clone()
    faces[10, 0], faces[333, 2], faces[m - 1, 1], faces[500, 1] = n, n + 8, -1, -8
    got, status, intact = _raw(case, faces=faces.reshape(-1).cuda())
    face = B.atlas_ref(m, 4)[2]
    hit = (face == 10) | (face == 333) | (face == m - 1) | (face == 500)
    print(f"status {status}, texels of the four faces {int(hit.sum())}, of them empty {int((got[3][hit] == -1).sum())}, "
          f"others that differ {int((got != plain)[:, ~hit].sum())}")
    assert status == 1 and intact
    assert bool((got[3][hit] == -1).all()) and bool((got[:3][:, hit] == 0.5).all()) and int(hit.sum()) == 10 + 6 + 6 + 10
    assert torch.equal(got[:, ~hit], plain[:, ~hit])
    with pytest.raises(ValueError, match=r"outside \[0, %d\)" % n):
        bake_texture(case["verts"].cuda(), case["cols"].cuda(), faces.cuda(), case["depth"].cuda(), case["colour"].cuda(), case["views"].cuda(), TAN,
                     patch=4, depth_tol=case["tol"])


def test_t2v_entrance_writes_a_textured_mesh_per_prompt(tmp_path):
    """Two prompts, 8 orbit views and the orbits at -40 and +40 deg, gs_mesh at 32^3 over the cube of half-width 1.2 (where the random-
    weight model's mesh has faces).  With gs_mesh_texture: a textured mesh per prompt whose geometry is the .ply's and whose texture has
    the atlas' size; every other output is that of the run without the key."""
    from tests.test_gs_depth_gpu import _entrance_cfg
    from videomv_amd.gs_mesh import load_mesh_obj, load_mesh_ply, texture_atlas
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    base = ["save_gaussians", "True", "gs_orbit_views", "8", "gs_mesh", "True", "gs_mesh_res", "32", "gs_mesh_extent", "1.2",
            "gs_mesh_elevations", "[-40, 40]"]
    runs = {}
    for name, extra in (("plain", base), ("texture", base + ["gs_mesh_texture", "True"])):
        cu = _entrance_cfg(tmp_path / name, extra)
        runs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    files = {k: sorted(os.path.relpath(os.path.join(d, f), r.log_dir) for d, _, fs in os.walk(r.log_dir) for f in fs) for k, r in runs.items()}
    new = [f for f in files["texture"] if f not in files["plain"]]
    assert [f for f in files["texture"] if f in files["plain"]] == files["plain"] and len(new) == 6
    assert sorted(f.rsplit("_gs_mesh", 1)[1] for f in new) == [".mtl", ".mtl", ".obj", ".obj", "_tex.png", "_tex.png"]
    assert len(runs["texture"].gs_exports) == len(runs["plain"].gs_exports) == 2
    for e, e0 in zip(runs["texture"].gs_exports, runs["plain"].gs_exports):
        assert "mesh_obj" not in e0 and e["mesh_fused_views"] == 24
        pv, _, pf = load_mesh_ply(e["mesh_ply"])
        verts, faces, uv, image = load_mesh_obj(e["mesh_obj"][:-4])
        T, want_uv = texture_atlas(pf.shape[0], 8)
        print(e["mesh_obj"], e["mesh_faces"], e["mesh_texture_size"], e["mesh_texels_baked"])
        assert torch.equal(verts, pv) and torch.equal(faces, pf) and pf.shape[0] > 0
        assert e["mesh_texture_size"] == T == image.shape[0] == image.shape[1] and float((uv - want_uv).abs().max()) <= 1e-4
        assert 0.0 < e["mesh_texels_baked"] <= 1.0
        # texels of no face are mid-grey, and the texels of faces are not all of one colour
        none = B.atlas_ref(pf.shape[0], 8)[2] >= pf.shape[0]
        assert bool((image[none] == 128).all()) and int(image[~none].reshape(-1, 3).unique(dim=0).shape[0]) > 16
    for f in files["plain"]:
        a, b = (os.path.join(runs[k].log_dir, f) for k in ("plain", "texture"))
        if f.endswith(".pt"):
            assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"]), f
        elif f.endswith((".ply", ".png", ".npy")):
            assert open(a, "rb").read() == open(b, "rb").read(), f
