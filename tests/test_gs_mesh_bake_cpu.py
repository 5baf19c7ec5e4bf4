"""Texture baking without a GPU: the ABI of vmv_gs_mesh_bake and its refusals, the closed-form atlas, the torch fallback of
``bake_texture`` against the fp64 restatement of tests/mesh_bake_ref.py on the cases the GPU tests bake, what the baked texture buys on the
analytic coloured sphere, the .obj writer and its inverse, and the entrance keys gs_mesh_texture / gs_mesh_texture_patch on the CPU plan
interpreter.  Every test prints its figures before it asserts (DESIGN.md §5.4 quotes them)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mesh_bake_ref as B
from tests import plan_interp
from tests.gs_tsdf_ref import TAN, f32, integrate_ref
from tests.test_gs_depth_cpu import _install_render_depth
from tests.test_gs_export_cpu import _files, _tiny_cfg
from tests.test_gs_mesh_cpu import MESH
from videomv_amd.gs_mesh import TsdfVolume, bake_texture, load_mesh_obj, load_mesh_ply, save_mesh_obj, texture_atlas


# ------------------------------------------------------------------------------------------------------------------------ ABI
def _params(**kw):
    """a valid block: 5 faces (3 cells, Wc = 2) at patch 8, T = 16; every pointer inside one host buffer, 8-byte aligned"""
    from videomv_amd import _lib as L
    keep = torch.zeros(4096, dtype=torch.int64)
    p = L.GsMeshBakeParams()
    base = keep.data_ptr()
    p.verts, p.vert_colours, p.faces, p.depth, p.colour, p.views, p.out, p.status = (base + 1024 * k for k in range(8))
    p.face_stride, p.n_faces, p.n_vertices, p.n_views, p.size = 3, 5, 7, 2, 16
    p.tan_half_fov, p.z_min, p.depth_tol, p.cos_min, p.patch, p.tex_size, p.plane_stride = 0.36, 0.05, 0.02, 0.1, 8, 16, 256
    for k, v in kw.items():
        setattr(p, k, v)
    return p, keep


POINTERS = ("verts", "vert_colours", "faces", "depth", "colour", "views", "out", "status")


def test_bake_params_abi_and_validation_without_a_device():
    """every refusal of the header's list and their order, none of which may touch a device (there is none here); a valid block is not
    tried: it would launch"""
    from videomv_amd import _lib as L
    lib = L.load()
    assert lib.vmv_abi_version() == L.ABI_VERSION == 12
    assert lib.vmv_sizeof(111) == C.sizeof(L.GsMeshBakeParams) == 128
    P = L.GsMeshBakeParams
    fields = ("verts", "vert_colours", "faces", "face_stride", "n_faces", "n_vertices", "depth", "colour", "views", "n_views", "size", "tan_half_fov",
              "z_min", "depth_tol", "cos_min", "patch", "tex_size", "out", "plane_stride", "status")
    assert [f for f, _ in P._fields_] == list(fields)
    assert [getattr(P, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84, 88, 92, 96, 100, 104, 112, 120]
    assert "vmv_gs_mesh_bake" in L.SYMBOLS and lib.vmv_sizeof(110) == 56 and lib.vmv_sizeof(109) == 88
    call = lambda p: lib.vmv_gs_mesh_bake(C.byref(p[0]), None)
    assert lib.vmv_gs_mesh_bake(None, None) == -3
    for field in POINTERS:
        assert call(_params(**{field: None})) == -3, field
    nan = float("nan")
    for bad in (dict(n_faces=0), dict(n_faces=-1), dict(n_vertices=0), dict(face_stride=2), dict(face_stride=-3), dict(n_views=0), dict(size=0),
                dict(tan_half_fov=0.0), dict(tan_half_fov=nan), dict(z_min=0.0), dict(z_min=-1.0), dict(depth_tol=0.0), dict(depth_tol=nan),
                dict(cos_min=-0.1), dict(cos_min=1.0), dict(cos_min=nan), dict(patch=3), dict(patch=0), dict(tex_size=8), dict(tex_size=24),
                dict(tex_size=0), dict(patch=4), dict(n_faces=9), dict(plane_stride=255), dict(plane_stride=0)):
        assert call(_params(**bad)) == -1, bad
    # the atlas' size follows n_faces and patch: 8 faces still fill 2 x 2 cells, 9 need 3 x 3
    assert call(_params(n_faces=9, tex_size=24, plane_stride=575)) == -1
    # VMV_ERANGE: a texture above 8192 (2 x 1025^2 faces at patch 8: T = 8200), an image above 32768, counts beyond int32
    big = dict(n_faces=2 * 1025 ** 2, tex_size=8200, plane_stride=8200 ** 2)
    assert call(_params(**big)) == -4
    assert call(_params(n_faces=2 * 1024 ** 2 + 1, tex_size=8200, plane_stride=8200 ** 2)) == -4       # one face past 1024^2 cells
    assert call(_params(size=32769)) == -4 and call(_params(n_vertices=2 ** 31)) == -4 and call(_params(n_vertices=2 ** 40)) == -4
    assert call(_params(n_faces=2 ** 31, patch=4, tex_size=4 * 32768, plane_stride=(4 * 32768) ** 2)) == -4
    # the order: null, invalid, range, alignment
    assert call(_params(n_faces=0, faces=None)) == -3 and call(_params(size=32769, face_stride=2)) == -1
    base = _params()[1].data_ptr()
    assert base % 8 == 0
    for field, off in (("faces", 4), ("faces", 2), ("verts", 2), ("vert_colours", 1), ("depth", 2), ("colour", 3), ("views", 2), ("out", 2), ("status", 1)):
        p = _params()
        setattr(p[0], field, getattr(p[0], field) + off)
        assert call(p) == -2, (field, off)
    assert call(_params(size=32769, faces=base + 2048 + 4)) == -4      # range before alignment
    assert call(_params(tex_size=8, out=base + 6 * 1024 + 2)) == -1    # invalid before alignment


# --------------------------------------------------------------------------------------------------------------------- the atlas
@pytest.mark.parametrize("P", [4, 5, 8])
@pytest.mark.parametrize("m", [1, 2, 3, 7, 864])
def test_atlas_properties(m, P):
    """T = P Wc with Wc the smallest square that holds ceil(m / 2) cells; every texel is owned by at most one face and the owned sets are
    the specified ones; the four taps of a bilinear lookup at 1 000 seeded points inside every face's UV triangle are texels of that face"""
    T, uv = texture_atlas(m, P)
    cells = (m + 1) // 2
    Wc = T // P
    assert T == P * Wc and Wc * Wc >= cells and (Wc - 1) ** 2 < cells
    assert uv.shape == (m, 3, 2) and uv.dtype == torch.float32
    # ownership, from the specification, texel by texel
    owner = torch.full((T, T), -1, dtype=torch.int64)
    claims = torch.zeros(T, T, dtype=torch.int64)
    for f in range(m):
        k = f // 2
        ox, oy = (k % Wc) * P, (k // Wc) * P
        for j in range(P):
            for i in range(P):
                if (i + j <= P - 1) if f % 2 == 0 else (i + j >= P):
                    owner[oy + j, ox + i] = f
                    claims[oy + j, ox + i] += 1
    assert int(claims.max()) == 1
    assert int((owner >= 0).sum()) == (m // 2) * P * P + (m % 2) * (P * (P + 1) // 2)
    _, _, face, s, t = B.atlas_ref(m, P)
    assert torch.equal(torch.where(face < m, face, torch.full_like(face, -1)), owner)
    # the UV triangle of every face in its own frame, and the flipped frame of the upper faces
    f = torch.arange(m)
    origin = torch.stack([(f // 2 % Wc) * P, (f // 2 // Wc) * P], dim=1).float()
    local = uv - origin[:, None]
    local = torch.where((f % 2 == 1)[:, None, None], P - local, local)
    assert torch.equal(local, torch.tensor([[0.5, 0.5], [P - 2.5, 0.5], [0.5, P - 2.5]]).expand(m, 3, 2))
    # bilinear taps: texel centres are half-integers, so a lookup at (x, y) touches columns floor(x - 0.5), + 1 and rows floor(y - 0.5), + 1
    gen = torch.Generator().manual_seed(1000 * m + P)
    bary = torch.rand(m, 1000, 3, generator=gen, dtype=torch.float64)
    bary = bary / bary.sum(-1, keepdim=True)
    pts = (bary[..., None] * uv.double()[:, None]).sum(2)                # [m, 1000, 2]
    x0, y0 = torch.floor(pts[..., 0] - 0.5).long(), torch.floor(pts[..., 1] - 0.5).long()
    for dx in (0, 1):
        for dy in (0, 1):
            x, y = x0 + dx, y0 + dy
            assert int(x.min()) >= 0 and int(y.min()) >= 0 and int(x.max()) < T and int(y.max()) < T
            assert torch.equal(owner[y, x], f[:, None].expand(m, 1000)), (dx, dy)


def test_atlas_refuses_a_texture_above_8192():
    assert texture_atlas(2 * 1024 ** 2, 8)[0] == 8192
    for m, P in ((2 * 1024 ** 2 + 1, 8), (2 * 256 ** 2 + 1, 32), (2 * 2048 ** 2 + 1, 4)):
        with pytest.raises(ValueError, match="smaller patch.*smaller gs_mesh_res"):
            texture_atlas(m, P)
    for m, P in ((0, 8), (10, 3)):
        with pytest.raises(ValueError, match="patch >= 4"):
            texture_atlas(m, P)


# ------------------------------------------------------------------------------------------------- the fallback against the reference
CASES = {"sphere-3-48-16-P4": (3, 48, 16, 4), "sphere-6-96-24-P8": (6, 96, 24, 8), "one-view-odd-patch": (1, 40, 17, 5),
         "odd-face-count": (3, 48, 16, 4, "odd"), "one-face": (3, 48, 16, 8, "one"), "degenerate-face": (3, 48, 16, 4, "degenerate")}


def bake(case, device="cpu", **kw):
    """``bake_texture`` on a case of tests/mesh_bake_ref.py, with the C floats the reference was given"""
    dev = lambda t: t.to(device)
    return bake_texture(dev(case["verts"]), dev(case["cols"]), dev(case["faces"]), dev(kw.pop("depth", case["depth"])), dev(kw.pop("colour", case["colour"])),
                        dev(kw.pop("views", case["views"])), f32(TAN), patch=case["P"], depth_tol=case["tol"], cos_min=f32(0.1), z_min=f32(0.05), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_fallback_matches_the_reference(name):
    case = B.sphere_bake_case(*CASES[name])
    tex, uv, info = bake(case)
    m = case["faces"].shape[0]
    assert tex.shape == (4, case["ref"]["T"], case["ref"]["T"]) and tex.dtype == torch.float32 and info["size"] == case["ref"]["T"]
    assert torch.equal(uv, texture_atlas(m, case["P"])[1])
    B.compare(name, tex, case)
    owned = int((case["ref"]["planes"][3] >= 0).sum())
    assert info["texels"] == owned == (m // 2) * case["P"] ** 2 + (m % 2) * (case["P"] * (case["P"] + 1) // 2)
    assert abs(info["baked"] + info["fallback"] - 1.0) < 1e-12 and info["baked"] == int((tex[3] > 0).sum()) / owned
    if name == "degenerate-face":                                       # its texels take the vertex colours, whatever the views see
        _, _, face, _, _ = B.atlas_ref(m, case["P"])
        assert bool((tex[3][face == 5] == 0).all()) and int((face == 5).sum()) > 0
    if name == "odd-face-count":                                        # the last cell has no upper face
        assert m % 2 == 1 and bool((tex[3][B.atlas_ref(m, case["P"])[2] == m] == -1).all())


def test_fallback_refuses_bad_input():
    case = B.sphere_bake_case(1, 40, 17, 5)
    for bad in (-1, case["verts"].shape[0], case["verts"].shape[0] + 8):
        faces = case["faces"].clone()
        faces[100, 1] = bad
        with pytest.raises(ValueError, match=r"outside \[0, %d\)" % case["verts"].shape[0]):
            bake_texture(case["verts"], case["cols"], faces, case["depth"], case["colour"], case["views"], TAN, patch=5, depth_tol=case["tol"])
    with pytest.raises(ValueError, match="cos_min"):
        bake_texture(case["verts"], case["cols"], case["faces"], case["depth"], case["colour"], case["views"], TAN, cos_min=1.0)
    with pytest.raises(ValueError, match="depth_tol"):
        bake_texture(case["verts"], case["cols"], case["faces"], case["depth"], case["colour"], case["views"], TAN, depth_tol=0.0)


# ------------------------------------------------------------------------------------------------- quality on the analytic sphere
@pytest.mark.parametrize("V,S,R,P", [(3, 48, 16, 4), (6, 96, 24, 8), (8, 128, 32, 8)])
def test_baked_texels_beat_the_vertex_colours(V, S, R, P):
    """The mean error of the baked texels against the TRUE colour of the sphere's surface under them is under half that of the
    interpolated vertex colours at the same texels, and over 0.8 of the texels of faces are baked.  Measured with this reference:
    (3, 48, 16, 4) 0.0933 against 0.2421 (0.385 of it), 0.861 baked; (6, 96, 24, 8) 0.0443 against 0.1860 (0.238), 0.909;
    (8, 128, 32, 8) 0.0294 against 0.1347 (0.218), 0.919."""
    case = B.sphere_bake_case(V, S, R, P)
    tex, _, info = bake(case)
    baked = tex[3] > 0
    true = B.surface_colour(case["ref"]["point"], case["centre"])
    e_baked = float((tex[:3].permute(1, 2, 0).double() - true)[baked].abs().mean())
    e_vertex = float((case["ref"]["vertex_rgb"] - true)[baked].abs().mean())
    print(f"(V, S, R, P) = ({V}, {S}, {R}, {P}): mean error of the baked texels {e_baked:.4f}, of the interpolated vertex colours {e_vertex:.4f} "
          f"(ratio {e_baked / e_vertex:.3f}), baked share {info['baked']:.3f}")
    assert e_baked < 0.5 * e_vertex
    assert info["baked"] > 0.8


# ------------------------------------------------------------------------------------------------------------------------ writer
def test_obj_round_trip_and_png_bytes(tmp_path):
    from PIL import Image
    case = B.sphere_bake_case(3, 48, 16, 4)
    tex, uv, _ = bake(case)
    stem = str(tmp_path / "ball_gs_mesh")
    n, m, T = save_mesh_obj(case["verts"], case["faces"], uv, tex, stem)
    assert (n, m, T) == (case["verts"].shape[0], 864, 84)
    assert sorted(os.listdir(tmp_path)) == ["ball_gs_mesh.mtl", "ball_gs_mesh.obj", "ball_gs_mesh_tex.png"]
    verts, faces, uv2, image = load_mesh_obj(stem)
    assert torch.equal(verts, case["verts"]) and torch.equal(faces, case["faces"])          # %.9g round-trips a float32
    assert uv2.shape == (m, 3, 2) and float((uv2 - uv).abs().max()) <= 1e-4
    want = (tex[:3].clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0)             # as save_mesh_ply rounds
    assert image.shape == (T, T, 3) and torch.equal(image, want)
    assert np.array_equal(np.array(Image.open(stem + "_tex.png")), want.numpy())
    obj = open(stem + ".obj").read().splitlines()
    assert obj[0] == "mtllib ball_gs_mesh.mtl" and obj[1] == "usemtl baked"
    kinds = [ln.split()[0] for ln in obj[2:]]
    assert kinds == ["v"] * n + ["vt"] * (3 * m) + ["f"] * m                                # vertices are not duplicated: per-corner UVs
    assert obj[2 + n + 3 * m] == "f %d/1 %d/2 %d/3" % tuple(int(i) + 1 for i in case["faces"][0])
    vt0 = [float(x) for x in obj[2 + n].split()[1:]]
    assert np.allclose(vt0, [0.5 / T, 1.0 - 0.5 / T], atol=1e-8)
    mtl = open(stem + ".mtl").read().split()
    assert mtl[:2] == ["newmtl", "baked"] and mtl[-2:] == ["map_Kd", "ball_gs_mesh_tex.png"]
    # the same inputs give the same files
    before = {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path)}
    save_mesh_obj(case["verts"], case["faces"], uv, tex, stem)
    assert before == {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path)}


# ------------------------------------------------------------------------------------------------------------------- entrance
BASE = ["save_gaussians", "True", "gs_fit_iters", "0"]


@pytest.mark.parametrize("extra", [["gs_orbit_views", "3", "gs_mesh_texture", "True"], ["gs_orbit_views", "3", "gs_mesh_texture_patch", "4"],
                                   MESH + ["gs_mesh_texture", "True", "gs_mesh_texture_patch", "3"], MESH + ["gs_mesh_texture_patch", "33"],
                                   MESH + ["gs_mesh_texture_patch", "6.5"], MESH + ["gs_mesh_texture_patch", "wide"]])
def test_texture_keys_are_refused_before_sampling(monkeypatch, tmp_path, extra):
    """either key without gs_mesh, a patch outside [4, 32] or not a whole number: refused, nothing sampled, nothing written"""
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, BASE + extra)
    with pytest.raises(Exception, match="gs_mesh_texture"):
        INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    assert not os.path.exists(tmp_path / "out")


def test_entrance_writes_a_textured_mesh_and_nothing_else_changes(monkeypatch, tmp_path):
    """3 orbit views of 32 px and the orbit at +50 deg, gs_mesh at 32^3 over the cube of half-width 1.2 (where the random model's mesh has
    faces).  With gs_mesh_texture: the three files next to the .ply, baked from the 6 fused views in fusion order with a depth tolerance
    of 2 voxels; every other file, the .ply included, is bit for bit that of the run without the key; the export draws no RNG."""
    from PIL import Image
    plan_interp.install(monkeypatch)
    _install_render_depth(monkeypatch)
    import videomv_amd.entrance  # noqa: F401
    from videomv_amd import gs_export, gs_mesh
    from videomv_amd.registry import INFER_ENGINE
    monkeypatch.setattr(TsdfVolume, "integrate", integrate_ref)
    fused, baked, rng = [], [], []

    plain_integrate = TsdfVolume.integrate

    def integrate(self, depth, cam_view, tan_half_fov, colour=None, **kw):
        fused.append((depth.clone(), colour.clone(), cam_view.clone()))
        plain_integrate(self, depth, cam_view, tan_half_fov, colour=colour, **kw)
    monkeypatch.setattr(TsdfVolume, "integrate", integrate)
    plain_bake = gs_mesh.bake_texture

    def bake_texture_spy(verts, colours, faces, depth, colour, cam_view, tan_half_fov, **kw):
        out = plain_bake(verts, colours, faces, depth, colour, cam_view, tan_half_fov, **kw)
        baked.append(dict(verts=verts, cols=colours, faces=faces, depth=depth, colour=colour, views=cam_view, tan=tan_half_fov, kw=kw, out=out))
        return out
    monkeypatch.setattr(gs_mesh, "bake_texture", bake_texture_spy)
    plain_export = gs_export._export_gaussians

    def export(*a, **k):
        before = torch.get_rng_state()
        rec = plain_export(*a, **k)
        rng.append(torch.equal(before, torch.get_rng_state()))
        return rec
    monkeypatch.setattr(gs_export, "_export_gaussians", export)
    mesh = BASE + MESH[:-1] + ["32", "gs_mesh_extent", "1.2", "gs_mesh_elevations", "[50]"]
    cfgs, n_fused = {}, {}
    for name, extra in (("plain", []), ("texture", ["gs_mesh_texture", "True"]), ("patch", ["gs_mesh_texture", "True", "gs_mesh_texture_patch", "5"])):
        cu = _tiny_cfg(tmp_path / name, mesh + extra)
        f0 = len(fused)
        cfgs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
        n_fused[name] = fused[f0:]
    assert rng == [True] * 3 and len(baked) == 2
    files = {k: _files(c.log_dir) for k, c in cfgs.items()}
    recs = {k: c.gs_exports[0] for k, c in cfgs.items()}
    assert not any(k in recs["plain"] for k in ("mesh_obj", "mesh_texture_size", "mesh_texels_baked"))
    new = [f for f in files["texture"] if f not in files["plain"]]
    assert [f for f in files["texture"] if f in files["plain"]] == files["plain"] == [f for f in files["patch"] if f in files["plain"]]
    assert len(new) == 3 and sorted(f.rsplit("_gs_mesh", 1)[1] for f in new) == [".mtl", ".obj", "_tex.png"]
    for name in ("texture", "patch"):
        for f in files["plain"]:                                        # every byte of every other file, the .ply mesh included
            a, b = (os.path.join(cfgs[k].log_dir, f) for k in ("plain", name))
            if f.endswith(".pt"):
                assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"]), f
            elif f.endswith(".png") and "_gs_orbit" in f:
                assert np.abs(np.array(Image.open(a)).astype(int) - np.array(Image.open(b)).astype(int)).max() <= 1      # as the existing tests
            elif f.endswith((".ply", ".png", ".npy")):
                assert open(a, "rb").read() == open(b, "rb").read(), f
    for name, call, P in (("texture", baked[0], 8), ("patch", baked[1], 5)):
        rec = recs[name]
        # every fused orbit, concatenated in fusion order; the depth tolerance is 2 voxels; the mesh is the one the .ply holds
        assert len(n_fused[name]) == 2 and rec["mesh_fused_views"] == 6
        for i, key in enumerate(("depth", "colour", "views")):
            assert torch.equal(call[key], torch.cat([f[i] for f in n_fused[name]])), key
        assert call["kw"] == dict(patch=P, depth_tol=2.0 * (2 * 1.2 / 32))
        pv, _, pf = load_mesh_ply(rec["mesh_ply"])
        assert torch.equal(call["verts"].cpu(), pv) and torch.equal(call["faces"].cpu(), pf) and pf.shape[0] > 0
        tex, uv, info = call["out"]
        verts, faces, uv2, image = load_mesh_obj(rec["mesh_obj"][:-4])
        assert rec["mesh_obj"].endswith("_gs_mesh.obj") and os.path.exists(rec["mesh_obj"])
        assert torch.equal(verts, pv) and torch.equal(faces, pf) and float((uv2 - uv).abs().max()) <= 1e-4
        T = texture_atlas(pf.shape[0], P)[0]
        assert rec["mesh_texture_size"] == T == image.shape[0] == image.shape[1] and rec["mesh_texels_baked"] == info["baked"]
        assert torch.equal(image, (tex[:3].clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0))
        # and the texture is the definition's: the fp64 reference on what the entrance passed
        case = B._case(dict(verts=call["verts"], cols=call["cols"], faces=call["faces"], depth=call["depth"], colour=call["colour"], views=call["views"],
                            P=P, tol=f32(call["kw"]["depth_tol"]), tan=f32(call["tan"])))
        print(name, rec["mesh_obj"], T, info)
        # (the random model's surface is a rough wall seen in 32-px views: 3.9 % of its texels have a decision within 1e-4 of its threshold)
        B.compare("entrance " + name, tex, case, need_both=False, max_unclear=None)
        assert 0.0 <= info["baked"] <= 1.0
