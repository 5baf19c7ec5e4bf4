"""Component labelling and the floater filter without a GPU: the ABI of vmv_gs_mesh_components and its refusals, the torch fallback of
``mesh_components`` against the sequential union-find of tests/mesh_cc_ref.py on every graph the GPU tests label, ``drop_small_components``
on hand-made meshes and on the analytic floater fixture, the entrance keys gs_mesh_min_component / gs_mesh_elevations on the CPU plan
interpreter, and what extra elevations do to the fused sphere (fp64 fusion reference)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R
from tests import plan_interp
from tests.gs_tsdf_ref import HALF, SPHERE, TAN, integrate_ref, pattern_colour, sphere_distance, spheres_depth
from tests.test_gs_depth_cpu import _install_render_depth
from tests.test_gs_export_cpu import _files, _tiny_cfg
from tests.test_gs_gpu import _cams
from tests.test_gs_mesh_cpu import MESH
from videomv_amd.gs_mesh import TsdfVolume, load_mesh_ply, mesh_stats


# ------------------------------------------------------------------------------------------------------------------------ ABI
def _params(**kw):
    from videomv_amd import _lib as L
    keep = torch.zeros(64, dtype=torch.int64)
    p = L.GsMeshComponentsParams()
    p.faces = keep.data_ptr()
    p.label, p.face_count, p.status = keep.data_ptr() + 128, keep.data_ptr() + 256, keep.data_ptr() + 384
    p.face_stride, p.n_faces, p.n_vertices = 3, 4, 16
    for k, v in kw.items():
        setattr(p, k, v)
    return p, keep


def test_components_params_abi_and_validation_without_a_device():
    """every refusal of the header's list, none of which may touch a device (there is none here); a valid block is not tried: it would launch"""
    from videomv_amd import _lib as L
    lib = L.load()
    assert lib.vmv_abi_version() == L.ABI_VERSION == 12
    assert lib.vmv_sizeof(110) == C.sizeof(L.GsMeshComponentsParams) == 56
    P = L.GsMeshComponentsParams
    assert [getattr(P, f).offset for f in ("faces", "face_stride", "n_faces", "n_vertices", "label", "face_count", "status")] == [0, 8, 16, 24, 32, 40, 48]
    assert "vmv_gs_mesh_components" in L.SYMBOLS and lib.vmv_sizeof(109) == 88
    call = lambda p: lib.vmv_gs_mesh_components(C.byref(p[0]), None)
    assert lib.vmv_gs_mesh_components(None, None) == -3
    for field in ("faces", "label", "face_count", "status"):
        assert call(_params(**{field: None})) == -3, field
    for bad in (dict(n_vertices=0), dict(n_vertices=-1), dict(n_faces=-1), dict(face_stride=2), dict(face_stride=0), dict(face_stride=-3)):
        assert call(_params(**bad)) == -1, bad
    assert call(_params(n_vertices=2 ** 31)) == -4 and call(_params(n_vertices=2 ** 40)) == -4         # VMV_ERANGE: int32 labels
    assert call(_params(n_vertices=0, faces=None)) == -3 and call(_params(n_vertices=2 ** 31, face_stride=2)) == -1      # the order: null, invalid, range
    base = _params()[1].data_ptr()
    assert base % 8 == 0
    for field, off in (("faces", 4), ("faces", 2), ("label", 2), ("face_count", 2), ("status", 1), ("status", 2)):
        p = _params()
        setattr(p[0], field, getattr(p[0], field) + off)
        assert call(p) == -2, (field, off)
    assert call(_params(n_vertices=2 ** 31, faces=base + 4)) == -4      # range before alignment


# ------------------------------------------------------------------------------------------------- the fallback against the reference
@pytest.mark.parametrize("name", R.CPU_CASES)
def test_fallback_matches_the_union_find(name):
    from videomv_amd.gs_mesh import mesh_components
    faces, n, label, count = R.case(name)
    got_label, got_count = mesh_components(faces, n)
    roots = int((label == torch.arange(n)).sum())
    print(f"{name}: {faces.shape[0]} faces, {n} vertices, {roots} components, largest {int(count.max())} faces")
    assert got_label.dtype == got_count.dtype == torch.int64 and got_label.shape == got_count.shape == (n,)
    assert torch.equal(got_label, label) and torch.equal(got_count, count)
    assert int(count.sum()) == faces.shape[0] and bool((count[label != torch.arange(n)] == 0).all())


def test_the_cases_are_what_they_claim():
    """the reference's own answers on the graphs whose answer is known in closed form"""
    for name in ("strip-forward", "strip-reverse", "strip-permuted", "hub"):
        _, n, label, count = R.case(name)
        assert bool((label == 0).all()) and int(count[0]) == 65536, name
    _, n, label, count = R.case("tetrahedra")
    assert torch.equal(label, torch.arange(n) % 4096) and bool((count[:4096] == 4).all()) and int(count[4096:].sum()) == 0
    _, n, label, count = R.case("bridge")
    assert bool((label[:702] == 0).all()) and bool((label[1000:] == 0).all()) and int(count[0]) == 1201
    assert torch.equal(label[702:1000], torch.arange(702, 1000))
    _, n, label, count = R.case("degenerate")
    assert label.tolist() == [0, 1, 2, 3, 1, 5, 1, 3, 8, 3, 8, 11, 12, 12, 12, 12, 12, 12, 12, 19]
    assert {r: int(c) for r, c in enumerate(count) if c} == {1: 3, 2: 1, 3: 2, 8: 1, 12: 4}
    _, n, label, count = R.case("floaters")
    assert n == 1800 and tuple(sorted(count[count > 0].tolist(), reverse=True)) == R.FLOATER_FACES


def test_winding_and_face_order_do_not_matter_and_bad_indices_raise():
    from videomv_amd.gs_mesh import mesh_components
    faces, n, label, count = R.case("random-257")
    gen = torch.Generator().manual_seed(3)
    shuffled = faces[torch.randperm(257, generator=gen)]
    shuffled = torch.stack([row[torch.randperm(3, generator=gen)] for row in shuffled])
    got = mesh_components(shuffled, n)
    assert torch.equal(got[0], label) and torch.equal(got[1], count)
    for bad in (-1, n, n + 8):
        f = faces.clone()
        f[100, 1] = bad
        with pytest.raises(ValueError, match=r"outside \[0, 300\)"):
            mesh_components(f, n)
    empty = mesh_components(faces[:0], 0)
    assert empty[0].shape == empty[1].shape == (0,)


# -------------------------------------------------------------------------------------------------------------- the floater filter
def _blobs():
    """three closed pieces with interleaved vertex numbers: an octahedron (8 faces; vertices 0, 3, 6, ...), and two tetrahedra (4 faces
    each; 1, 4, 7, 10 and 2, 5, 8, 11), three isolated vertices (13, 14, 16) -> (verts [17, 3], colours, faces [16, 3])"""
    octa = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]) * 3
    tet = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]) * 3
    faces = torch.cat([tet + 1, octa, tet + 2])[torch.tensor([5, 0, 9, 12, 1, 6, 13, 2, 7, 14, 3, 8, 15, 4, 10, 11])]
    gen = torch.Generator().manual_seed(1)
    return torch.randn(17, 3, generator=gen), torch.rand(17, 3, generator=gen), faces


def test_drop_small_components_on_hand_made_blobs():
    from videomv_amd.gs_mesh import drop_small_components
    verts, cols, faces = _blobs()
    # thresholds of 0: the identity (the isolated vertices stay too)
    v, c, f, info = drop_small_components(verts, cols, faces)
    assert torch.equal(v, verts) and torch.equal(c, cols) and torch.equal(f, faces)
    assert info == dict(components=6, kept=6, largest_faces=8, dropped_faces=0, dropped_vertices=0)
    # min_faces decides alone: 1 drops the isolated vertices only, 5 the tetrahedra, 9 everything
    for min_faces, kept, faces_left, verts_left in ((1, 3, 16, 14), (4, 3, 16, 14), (5, 1, 8, 6), (8, 1, 8, 6), (9, 0, 0, 0)):
        v, c, f, info = drop_small_components(verts, cols, faces, min_faces=min_faces)
        assert (info["kept"], f.shape[0], v.shape[0]) == (kept, faces_left, verts_left), min_faces
    # min_fraction decides alone: the tetrahedra hold exactly half the largest count
    for frac, kept in ((0.5, 3), (0.51, 1), (1.0, 1), (1e-9, 3)):
        assert drop_small_components(verts, cols, faces, min_fraction=frac)[3]["kept"] == kept, frac
    # order kept, remap valid: the kept faces name the same positions and colours as before, in the same order
    for kw in (dict(min_faces=5), dict(min_faces=1), dict(min_fraction=0.4)):
        v, c, f, info = drop_small_components(verts, cols, faces, **kw)
        want = R.drop_ref(verts.numpy(), cols.numpy(), faces.numpy(), **kw)
        assert np.array_equal(v.numpy(), want[0]) and np.array_equal(c.numpy(), want[1]) and np.array_equal(f.numpy(), want[2]) and info == want[3]
        keep_f = torch.tensor([bool((verts[face][:, None] == v[None]).all(-1).any(-1).all()) for face in faces])
        assert torch.equal(v[f], verts[faces[keep_f]]) and torch.equal(c[f], cols[faces[keep_f]])
        assert f.dtype == torch.int64 and (f.numel() == 0 or (int(f.min()) >= 0 and int(f.max()) < v.shape[0]))
    # a tie for largest: both tetrahedra stay at min_fraction 1 once the octahedron is gone
    two = faces[(faces % 3 != 0).all(1)]
    v, c, f, info = drop_small_components(verts, cols, two, min_fraction=1.0, min_faces=1)
    assert info == dict(components=11, kept=2, largest_faces=4, dropped_faces=0, dropped_vertices=9) and torch.equal(v[f], verts[two])
    # an empty mesh, with and without vertices
    v, c, f, info = drop_small_components(verts[:0], cols[:0], faces[:0], min_fraction=0.5, min_faces=3)
    assert v.shape == c.shape == f.shape == (0, 3) and info == dict(components=0, kept=0, largest_faces=0, dropped_faces=0, dropped_vertices=0)
    v, c, f, info = drop_small_components(verts, cols, faces[:0], min_faces=1)
    assert v.shape == (0, 3) and f.shape == (0, 3) and info["components"] == 17 and info["dropped_vertices"] == 17


def test_floater_fixture_keeps_the_object_and_its_large_neighbour():
    """six balls through surface_nets: 1 800 vertices, 3 576 faces in components of 3 052, 188, 124, 92, 72 and 48 faces; min_fraction
    0.05 (152.6 faces) keeps the first two: two closed oriented spheres, Euler characteristic 4"""
    from videomv_amd.gs_mesh import drop_small_components
    verts, cols, faces = R.floater_mesh()
    assert verts.shape == (1800, 3) and faces.shape == (3576, 3)
    v, c, f, info = drop_small_components(verts, cols, faces, min_fraction=0.05)
    st = mesh_stats(v, f)
    print(info, st)
    assert info == dict(components=6, kept=2, largest_faces=3052, dropped_faces=336, dropped_vertices=1800 - v.shape[0])
    assert f.shape[0] == 3240 and st["open_edges"] == 0 and st["misoriented"] == 0 and st["euler"] == 4 and st["vertices"] == v.shape[0]
    want = R.drop_ref(verts.numpy(), cols.numpy(), faces.numpy(), min_fraction=0.05)
    assert np.array_equal(v.numpy(), want[0]) and np.array_equal(c.numpy(), want[1]) and np.array_equal(f.numpy(), want[2])
    # every kept vertex lies on one of the two kept balls, to the quarter voxel of test_surface_nets_sphere
    assert float(sphere_distance(v, R.BALLS[:1] + R.BALLS[3:4]).max()) <= 0.25 * 1.6 / 32


# ------------------------------------------------------------------------------------------------------------------- entrance
BASE = ["save_gaussians", "True", "gs_fit_iters", "0"]


@pytest.mark.parametrize("extra", [["gs_orbit_views", "3", "gs_mesh_min_component", "0.1"], ["gs_orbit_views", "3", "gs_mesh_elevations", "[40]"],
                                   MESH + ["gs_mesh_min_component", "1.5"], MESH + ["gs_mesh_min_component", "-0.1"],
                                   MESH + ["gs_mesh_min_component", "half"], MESH + ["gs_mesh_elevations", "40"],
                                   MESH + ["gs_mesh_elevations", "[90]"], MESH + ["gs_mesh_elevations", "[10, -90]"],
                                   MESH + ["gs_mesh_elevations", "[10, .nan]"], MESH + ["gs_mesh_elevations", "[10, up]"]])
def test_component_and_elevation_keys_are_refused_before_sampling(monkeypatch, tmp_path, extra):
    """either key without gs_mesh, a fraction outside [0, 1] or not a number, elevations that are not a list of finite numbers inside
    (-90, 90): refused, nothing sampled, nothing written"""
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, BASE + extra)
    with pytest.raises(Exception, match="gs_mesh_min_component|gs_mesh_elevations"):
        INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    assert not os.path.exists(tmp_path / "out")


def test_entrance_fuses_extra_elevations_and_drops_components(monkeypatch, tmp_path):
    """3 orbit views of 32 px, gs_mesh at 32^3 over the cube of half-width 1.2 (test_t2v_entrance_exports_a_mesh says why).  With gs_mesh_elevations [-50, 50]: three render_depth calls of (1, 3), three fusion calls,
    9 views fused, and every file but the mesh is that of the run without the key.  With gs_mesh_min_component: the written mesh is the
    reference filter of the mesh of the run without it (the analytic floater fixture is appended to every extracted mesh: the random
    model's own is a single piece)."""
    plan_interp.install(monkeypatch)
    calls = _install_render_depth(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    fused = []

    def integrate(self, depth, cam_view, tan_half_fov, colour=None, **kw):
        fused.append((tuple(depth.shape), tuple(cam_view.shape), tuple(colour.shape), cam_view.float().cpu().clone()))
        integrate_ref(self, depth, cam_view, tan_half_fov, colour=colour, **kw)
    monkeypatch.setattr(TsdfVolume, "integrate", integrate)
    plain_extract = TsdfVolume.extract

    def extract(self, *a, **k):
        # the random model's mesh is one piece: the six analytic balls ride along, so that the filter has something to drop
        v, c, f = plain_extract(self, *a, **k)
        bv, bc, bf = R.floater_mesh()
        return torch.cat([v, bv]), torch.cat([c, bc]), torch.cat([f, bf + v.shape[0]])
    monkeypatch.setattr(TsdfVolume, "extract", extract)
    from videomv_amd import lgm as _lgm
    plain_orbit, orbits = _lgm.orbit_cameras, []

    def orbit_cameras(camera_data, num_views, elevation, camera_distance, opt=None):
        out = plain_orbit(camera_data, num_views, elevation, camera_distance, opt)
        orbits.append((int(num_views), float(elevation), float(camera_distance), out[0][0].float().clone()))
        return out
    monkeypatch.setattr(_lgm, "orbit_cameras", orbit_cameras)
    runs = (("mesh", []), ("elev", ["gs_mesh_elevations", "[-50, 50]"]), ("both", ["gs_mesh_elevations", "[-50, 50]", "gs_mesh_min_component", "0.3"]))
    cfgs, n_calls = {}, {}
    for name, extra in runs:
        cu = _tiny_cfg(tmp_path / name, BASE + MESH[:-1] + ["32", "gs_mesh_extent", "1.2"] + extra)     # the cube where the random model's mesh has faces
        c0, f0, o0 = len(calls), len(fused), len(orbits)
        cfgs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
        n_calls[name] = (calls[c0:], fused[f0:], orbits[o0:])
    recs = {k: c.gs_exports[0] for k, c in cfgs.items()}
    for name, n in (("mesh", 1), ("elev", 3), ("both", 3)):
        rendered, fusions, cams = n_calls[name]
        assert rendered == [(1, 3)] * n and len(fusions) == n and recs[name]["mesh_fused_views"] == 3 * n
        assert all(f[:3] == ((3, 32, 32), (3, 4, 4), (3, 3, 32, 32)) for f in fusions)
        # the entrance's own orbit first, then one orbit_cameras orbit per extra elevation in the order given, same views, same distance;
        # each fusion call sees the cameras of its own orbit
        assert [c[:3] for c in cams] == [(3, e, cams[0][2]) for e in ([cams[0][1]] + [-50.0, 50.0])[:n]]
        assert all(torch.equal(f[3], c[3]) for f, c in zip(fusions, cams))
    assert torch.equal(n_calls["elev"][1][0][3], n_calls["mesh"][1][0][3]) and not torch.equal(n_calls["elev"][1][1][3], n_calls["elev"][1][2][3])
    # every non-mesh file is that of the run without the keys
    files = {k: _files(c.log_dir) for k, c in cfgs.items()}
    from PIL import Image
    for name in ("elev", "both"):
        assert files[name] == files["mesh"]
        for f in files["mesh"]:
            a, b = (os.path.join(cfgs[k].log_dir, f) for k in ("mesh", name))
            if f.endswith(".pt"):
                assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"])
            elif f.endswith(".png") and "_gs_orbit" in f:
                assert np.abs(np.array(Image.open(a)).astype(int) - np.array(Image.open(b)).astype(int)).max() <= 1      # as the existing test
            elif f.endswith((".ply", ".png", ".npy")) and not f.endswith("_gs_mesh.ply"):
                assert open(a, "rb").read() == open(b, "rb").read(), f
    # gs_mesh_min_component: the reference filter of the unfiltered run's mesh, and counts that describe what was written
    for plain, dropped in (("elev", "both"),):
        v0, rgb0, f0 = load_mesh_ply(recs[plain]["mesh_ply"])
        v1, rgb1, f1 = load_mesh_ply(recs[dropped]["mesh_ply"])
        want = R.drop_ref(v0.numpy(), rgb0.numpy(), f0.numpy(), min_fraction=0.3)
        print(plain, dropped, want[3], recs[dropped])
        assert np.array_equal(v1.numpy(), want[0]) and np.array_equal(rgb1.numpy(), want[1]) and np.array_equal(f1.numpy(), want[2])
        rec = recs[dropped]
        assert rec["mesh_components"] == want[3]["components"] and rec["mesh_components_dropped"] == want[3]["components"] - want[3]["kept"]
        assert rec["mesh_vertices"] == v1.shape[0] and rec["mesh_faces"] == f1.shape[0] and rec["mesh_open_edges"] == mesh_stats(v1, f1)["open_edges"]
        assert "mesh_components" not in recs[plain] and "mesh_components_dropped" not in recs[plain]
        assert f0.shape[0] > 3576 and want[3]["components"] >= 7 and want[3]["kept"] == 1 and f1.shape[0] == 3052 and rec["mesh_open_edges"] == 0


# ------------------------------------------------------------------------------------------------------- what extra elevations buy
def test_extra_elevations_fix_the_caps_of_the_fused_sphere():
    """SPHERE seen by 12 cameras of 96 px at elevation 15 deg, fused at R = 32 by the fp64 reference: worst vertex 0.779 voxel from the
    sphere, at the cap the orbit sees at a grazing angle.  With the orbits at -50 and +50 deg fused too: 0.358 voxel, asserted <= 0.5;
    closed, oriented, genus 0.  The volume deficit stays (-3.05 % -> -3.72 %): it is the shrinkage of surface nets, not the caps."""
    worst = {}
    for name, elevations in (("one", (15.0,)), ("three", (15.0, -50.0, 50.0))):
        vol = TsdfVolume(32, HALF, device="cpu")
        for e in elevations:
            cv, _ = _cams(12, elevation=e)
            integrate_ref(vol, spheres_depth(cv, 96, SPHERE).float(), cv, TAN, colour=pattern_colour(12, 96))
        verts, _, faces = vol.extract()
        st = mesh_stats(verts, faces)
        worst[name] = float(sphere_distance(verts, SPHERE).max()) / vol.voxel
        print(name, st, f"worst vertex distance {worst[name]:.3f} voxel, volume {100 * (st['volume'] / (4 / 3 * np.pi * 0.32 ** 3) - 1):+.2f} %")
        assert vol.n_views == 12 * len(elevations)
        assert st["euler"] == 2 and st["open_edges"] == 0 and st["misoriented"] == 0
    assert worst["three"] <= 0.5 and worst["one"] > 0.5
