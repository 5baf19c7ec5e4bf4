"""Component labelling on the device (csrc/gs_mesh_cc.hip through vmv_gs_mesh_components and gs_mesh.mesh_components) against the
sequential union-find of tests/mesh_cc_ref.py (checked against closed forms in tests/test_gs_mesh_cc_cpu.py): labels and counts are
integers and must be EQUAL.  The graphs are the ones at which a concurrent union-find can go wrong (long chains in three numberings,
one contended address, interleaved numbering, a bridge listed last, degenerate and duplicate faces, a partial last block), then
determinism, the store and read footprints, out-of-range indices, and the entrance keys gs_mesh_elevations / gs_mesh_min_component.

Every raw call writes into int32 buffers with 64 guard elements of a pattern on each side of label, face_count and status: a store
outside the outputs, or a read of the parent array at an index that escaped the range test, shows as a changed guard or a wrong label,
not as a fault."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mesh_cc_ref as R
from tests.gs_tsdf_ref import TAN, sphere_case

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0x5A5A5A5A


def _raw(faces_buf, n_faces, n, stride=3, offset=0):
    """one call of vmv_gs_mesh_components on the current stream: faces at ``faces_buf`` (int64, on the device) + ``offset`` elements,
    outputs inside one guarded int32 buffer  G | label n | G | face_count n | G | status | G  -> (label, face_count, status, guards_intact)"""
    from videomv_amd import _lib as L
    from videomv_amd.ops import _stream_ptr
    assert faces_buf.dtype == torch.int64 and faces_buf.is_cuda and faces_buf.is_contiguous()
    assert n_faces == 0 or offset + (n_faces - 1) * stride + 3 <= faces_buf.numel()              # bounds of the read, checked before the launch
    total = 4 * GUARD + 2 * n + 1
    buf = torch.full((total,), PATTERN, dtype=torch.int32, device="cuda")
    at = {"label": GUARD, "face_count": 2 * GUARD + n, "status": 3 * GUARD + 2 * n}
    p = L.GsMeshComponentsParams()
    p.faces, p.face_stride, p.n_faces, p.n_vertices = faces_buf.data_ptr() + 8 * offset, stride, n_faces, n
    p.label, p.face_count, p.status = (buf.data_ptr() + 4 * at[k] for k in ("label", "face_count", "status"))
    L.check(L.load().vmv_gs_mesh_components(C.byref(p), _stream_ptr()), "gs_mesh_components")
    torch.cuda.synchronize()
    out = buf.cpu()
    payload = torch.zeros(total, dtype=torch.bool)
    payload[at["label"]:at["label"] + n] = payload[at["face_count"]:at["face_count"] + n] = True
    payload[at["status"]] = True
    return (out[at["label"]:at["label"] + n].long(), out[at["face_count"]:at["face_count"] + n].long(), int(out[at["status"]]),
            bool((out[~payload] == PATTERN).all()))


def _dense(faces):
    """a device buffer that holds at least one element, for the case without faces (the launcher refuses a null pointer)"""
    return faces.reshape(-1).cuda() if faces.numel() else torch.zeros(3, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("name", R.CPU_CASES)
def test_kernel_matches_the_union_find(name):
    from videomv_amd.gs_mesh import mesh_components
    faces, n, label, count = R.case(name)
    got_label, got_count, status, intact = _raw(_dense(faces), faces.shape[0], n)
    print(f"{name}: {faces.shape[0]} faces, {n} vertices, {int((label == torch.arange(n)).sum())} components, status {status}, "
          f"labels that differ {int((got_label != label).sum())}, counts that differ {int((got_count != count).sum())}")
    assert status == 0 and intact
    assert torch.equal(got_label, label) and torch.equal(got_count, count)
    dev_label, dev_count = mesh_components(faces.cuda(), n)
    assert dev_label.is_cuda and dev_label.dtype == dev_count.dtype == torch.int64
    assert torch.equal(dev_label.cpu(), label) and torch.equal(dev_count.cpu(), count)


def _device_mesh():
    """the mesh TsdfVolume.extract gives on the device for the two-spheres case -> faces (on the device), n"""
    from videomv_amd.gs_mesh import TsdfVolume
    case = sphere_case(8, 64, 32, "two", 0.45)
    vol = TsdfVolume(32, 0.45, device="cuda")
    vol.integrate(case["depth"], case["views"], TAN, colour=case["colour"])
    verts, _, faces = vol.extract()
    return faces, int(verts.shape[0])


def test_mesh_extracted_on_the_device():
    from videomv_amd.gs_mesh import drop_small_components, mesh_components
    faces, n = _device_mesh()
    assert faces.is_cuda and faces.dtype == torch.int64 and faces.shape[0] > 500
    label, count = R.components_ref(faces.cpu().numpy(), n)
    got_label, got_count, status, intact = _raw(faces.contiguous().reshape(-1), faces.shape[0], n)
    print(f"two spheres: {faces.shape[0]} faces, {n} vertices, components of {sorted(count[count > 0].tolist(), reverse=True)} faces")
    assert status == 0 and intact and np.array_equal(got_label.numpy(), label) and np.array_equal(got_count.numpy(), count)
    assert int((count > 0).sum()) >= 2                                  # the two spheres do not touch
    dev = mesh_components(faces, n)
    assert np.array_equal(dev[0].cpu().numpy(), label) and np.array_equal(dev[1].cpu().numpy(), count)
    # the floater filter on the device against the reference filter
    verts = torch.arange(3 * n, dtype=torch.float32, device="cuda").reshape(n, 3)
    v, c, f, info = drop_small_components(verts, verts * 0.5, faces, min_fraction=0.9)
    want = R.drop_ref(verts.cpu().numpy(), (verts * 0.5).cpu().numpy(), faces.cpu().numpy(), min_fraction=0.9)
    assert v.is_cuda and f.is_cuda and info == want[3]
    assert np.array_equal(v.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1]) and np.array_equal(f.cpu().numpy(), want[2])


@pytest.mark.parametrize("name", ["strip-forward", "strip-reverse", "strip-permuted", "hub", "device-mesh"])
def test_two_runs_and_any_face_order_give_the_same_bits(name):
    if name == "device-mesh":
        faces, n = _device_mesh()
        faces = faces.cpu()
    else:
        faces, n = R.case(name)[:2]
    buf = faces.reshape(-1).cuda()
    a, b = _raw(buf, faces.shape[0], n), _raw(buf.clone(), faces.shape[0], n)
    assert a[2] == b[2] == 0 and a[3] and b[3] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a seeded shuffle of the faces and of every face's winding: the same labels and counts
    gen = torch.Generator().manual_seed(17)
    m = faces.shape[0]
    shuffled = faces[torch.randperm(m, generator=gen)]
    shuffled = torch.gather(shuffled, 1, torch.rand(m, 3, generator=gen).argsort(dim=1))
    assert not torch.equal(shuffled, faces) and torch.equal(shuffled.sort(dim=1).values.unique(dim=0), faces.sort(dim=1).values.unique(dim=0))
    c = _raw(shuffled.reshape(-1).cuda(), m, n)
    assert c[2] == 0 and c[3] and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


def test_strided_faces_read_nothing_but_their_indices():
    """face_stride 5 inside an int64 buffer whose padding holds 2^62, the first face 7 elements in: the result of the dense call, status 0
    (a read of the padding would flag an index out of range)"""
    for name in ("random-257", "floaters"):
        faces, n, label, count = R.case(name)
        m = faces.shape[0]
        buf = torch.full((7 + 5 * m + 9,), 2 ** 62, dtype=torch.int64)
        buf[7:7 + 5 * m].view(m, 5)[:, :3] = faces
        got = _raw(buf.cuda(), m, n, stride=5, offset=7)
        assert got[2] == 0 and got[3] and torch.equal(got[0], label) and torch.equal(got[1], count), name
    # the host layer passes a strided view through as it is
    from videomv_amd.gs_mesh import mesh_components
    faces, n, label, count = R.case("random-257")
    wide = torch.full((257, 5), 2 ** 62, dtype=torch.int64)
    wide[:, :3] = faces
    dev = mesh_components(wide.cuda()[:, :3], n)
    assert torch.equal(dev[0].cpu(), label) and torch.equal(dev[1].cpu(), count)


def test_out_of_range_indices_are_skipped_and_flagged():
    """-1, -8, n and n + 8 (all within the guards' reach) in four faces, one of them the only bridge between two pieces: status bit 0,
    those faces neither counted nor connected, guards intact; mesh_components raises"""
    from videomv_amd.gs_mesh import mesh_components
    faces, n = R.case("bridge")[:2]
    faces = faces.clone()
    m = faces.shape[0]
    faces[m - 1, 1] = -1                                               # the bridge itself
    faces[10, 0], faces[700 + 20, 2], faces[300, 1] = n, n + 8, -8
    label, count = R.components_ref(faces.numpy(), n)
    assert int(count.sum()) == m - 4 and label[1000] == 1000 and int(count[0]) < 700          # the reference skipped them: two pieces, and more
    got_label, got_count, status, intact = _raw(faces.reshape(-1).cuda(), m, n)
    print(f"status {status}, labels that differ {int((got_label.numpy() != label).sum())}, faces counted {int(got_count.sum())} of {m}")
    assert status == 1 and intact
    assert np.array_equal(got_label.numpy(), label) and np.array_equal(got_count.numpy(), count)
    with pytest.raises(ValueError, match=r"outside \[0, 1502\)"):
        mesh_components(faces.cuda(), n)
    # all faces bad: identity labels, zero counts
    bad = torch.full((5, 3), -1, dtype=torch.int64)
    got = _raw(bad.reshape(-1).cuda(), 5, 9)
    assert got[2] == 1 and got[3] and torch.equal(got[0], torch.arange(9)) and int(got[1].sum()) == 0


def test_t2v_entrance_fuses_extra_elevations_and_drops_components(tmp_path):
    """Two prompts, 8 orbit views, gs_mesh at 32^3 over the cube of half-width 1.2 (where the random-weight model's mesh has faces:
    test_t2v_entrance_exports_a_mesh).  Run A adds the orbits at -40 and +40 deg: 24 views fused.  Run B is A plus
    gs_mesh_min_component 0.05: its mesh is the reference filter of A's, its counts say so, and every other file is A's."""
    from tests.test_gs_depth_gpu import _entrance_cfg
    from videomv_amd.gs_mesh import load_mesh_ply, mesh_stats
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    base = ["save_gaussians", "True", "gs_orbit_views", "8", "gs_mesh", "True", "gs_mesh_res", "32", "gs_mesh_extent", "1.2",
            "gs_mesh_elevations", "[-40, 40]"]
    runs = {}
    for name, extra in (("A", base), ("B", base + ["gs_mesh_min_component", "0.05"])):
        cu = _entrance_cfg(tmp_path / name, extra)
        runs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    files = {k: sorted(os.path.relpath(os.path.join(d, f), r.log_dir) for d, _, fs in os.walk(r.log_dir) for f in fs) for k, r in runs.items()}
    assert files["A"] == files["B"] and len(runs["A"].gs_exports) == len(runs["B"].gs_exports) == 2
    for ea, eb in zip(runs["A"].gs_exports, runs["B"].gs_exports):
        assert ea["mesh_fused_views"] == eb["mesh_fused_views"] == 24
        assert "mesh_components" not in ea and "mesh_components_dropped" not in ea
        va, rgba, fa = load_mesh_ply(ea["mesh_ply"])
        vb, rgbb, fb = load_mesh_ply(eb["mesh_ply"])
        want = R.drop_ref(va.numpy(), rgba.numpy(), fa.numpy(), min_fraction=0.05)
        print(ea["mesh_ply"], ea["mesh_vertices"], ea["mesh_faces"], want[3], {k: v for k, v in eb.items() if k.startswith("mesh") and k != "mesh_ply"})
        assert ea["mesh_faces"] == fa.shape[0] > 0 and ea["mesh_vertices"] == va.shape[0]
        assert np.array_equal(vb.numpy(), want[0]) and np.array_equal(rgbb.numpy(), want[1]) and np.array_equal(fb.numpy(), want[2])
        assert eb["mesh_components"] == want[3]["components"] and eb["mesh_components_dropped"] == want[3]["components"] - want[3]["kept"]
        assert eb["mesh_vertices"] == vb.shape[0] == va.shape[0] - want[3]["dropped_vertices"]
        assert eb["mesh_faces"] == fb.shape[0] == fa.shape[0] - want[3]["dropped_faces"]
        assert eb["mesh_open_edges"] == mesh_stats(vb, fb)["open_edges"] and ea["mesh_open_edges"] == mesh_stats(va, fa)["open_edges"]
    for f in files["A"]:
        a, b = (os.path.join(runs[k].log_dir, f) for k in ("A", "B"))
        if f.endswith(".pt"):
            assert torch.equal(torch.load(a)["latent"], torch.load(b)["latent"]), f
        elif f.endswith((".ply", ".png", ".npy")) and not f.endswith("_gs_mesh.ply"):
            assert open(a, "rb").read() == open(b, "rb").read(), f
