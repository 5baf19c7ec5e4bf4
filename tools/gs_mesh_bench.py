"""ms per call of the TSDF fusion kernel (csrc/gs_tsdf.hip through gs_mesh.TsdfVolume.integrate) and of the mesh extraction
(TsdfVolume.extract: the field + surface nets in torch on the device), on median-depth maps rendered from a seeded scene of 65 536
Gaussians seen from V orbit views: (R, V, S) = (128, 24, 256) and (256, 48, 512) by default.  Next to the kernel's time, what it
replaces: a torch-eager formulation of the same definition on the same GPU in the same process, one view at a time over the whole
volume (it states the alternative; it is not a target).  Medians over --iters calls after --warmup.  Rates: the depth gathers the
kernel issues (R^3 V, one per voxel and view) per second, and the plane bytes it moves (7 planes x R^3 x 4 B, read and written) per
second.  Prints one JSON line per shape; --log FILE appends them to FILE.
    python tools/gs_mesh_bench.py [--shapes 128:24:256,256:48:512] [--iters 30] [--warmup 5] [--gaussians 65536]
--components measures the component labelling instead (csrc/gs_mesh_cc.hip), on the meshes extracted at those shapes and on a strip of
65 536 triangles numbered by a seeded permutation: the median ms of one vmv_gs_mesh_components call into preallocated outputs, of the
eager propagation that is gs_mesh.mesh_components' CPU fallback run on the device in the same process (the yardstick; it states the
alternative), and of gs_mesh.drop_small_components (labelling, status read-back, masks and the remap).  Appends to
profiles/gs_mesh_cc_bench.log unless --log names another file.
    python tools/gs_mesh_bench.py --components [--shapes ...] [--iters 30] [--warmup 5]
--bake measures the texture baking instead (csrc/gs_mesh_bake.hip), on the meshes extracted at those shapes, baked from the V views they
were fused from at patch 8 (or the largest patch below it whose atlas fits a texture of 8192) with a depth tolerance of 2 voxels: the median ms of one vmv_gs_mesh_bake call into preallocated planes, and of
the torch restatement that is gs_mesh.bake_texture's CPU fallback run on the device in the same process (the yardstick; it states the
alternative).  Rates: texel-view evaluations (texels of faces x V) per second and the plane bytes written (4 planes x T^2 x 4 B) per second.
Appends to profiles/gs_mesh_bake_bench.log unless --log names another file.
    python tools/gs_mesh_bench.py --bake [--shapes ...] [--patch 8] [--iters 30] [--warmup 5]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gs_fit_bench import median_ms, orbit, scene  # noqa: E402


def eager_integrate(acc, depth, colour, views, tan, origin, voxel, trunc, z_min, carve):
    """the definition of include/vmv.h ("TSDF fusion") in torch eager, fp32 on the device, a view at a time; acc [7, R, R, R] in place"""
    R, S = acc.shape[-1], depth.shape[-1]
    i = torch.arange(R, dtype=torch.float32, device=acc.device)
    wz, wy, wx = torch.meshgrid(origin[2] + i * voxel, origin[1] + i * voxel, origin[0] + i * voxel, indexing="ij")
    for v, m in enumerate(views):                                       # m: 16 Python floats (no device read in the loop)
        xv = wx * m[0] + wy * m[4] + wz * m[8] + m[12]
        yv = wx * m[1] + wy * m[5] + wz * m[9] + m[13]
        z = wx * m[2] + wy * m[6] + wz * m[10] + m[14]
        zt = z * tan
        fx, fy = torch.floor(((xv / zt + 1) * S - 1) * 0.5 + 0.5), torch.floor(((yv / zt + 1) * S - 1) * 0.5 + 0.5)
        seen = (z > z_min) & (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
        pix = torch.nan_to_num(fy, nan=0.0).clamp(0, S - 1).long() * S + torch.nan_to_num(fx, nan=0.0).clamp(0, S - 1).long()
        d = depth[v].reshape(-1)[pix]
        sdf = d - z
        surf = seen & (d > 0)
        behind = surf & (sdf < -trunc)
        fused = surf & ~behind
        free = seen & (d == 0) if carve else torch.zeros_like(seen)
        acc[2] += behind
        acc[0] += torch.where(fused, (sdf / trunc).clamp(max=1.0), free.to(torch.float32))
        acc[1] += fused | free
        if colour is not None:
            near = fused & (sdf <= trunc)
            acc[3:6] += colour[v].reshape(3, -1)[:, pix] * near
            acc[6] += near


def components_record(name, verts, cols, faces, iters, warmup):
    """-> the JSON record of one mesh: kernel, eager propagation and floater filter, and that the first two agree"""
    from videomv_amd import _lib as L
    from videomv_amd.gs_mesh import _components_eager, drop_small_components
    from videomv_amd.ops import _stream_ptr
    n, m = int(verts.shape[0]), int(faces.shape[0])
    faces = faces.contiguous()
    out = torch.empty(2 * n + 1, dtype=torch.int32, device="cuda")
    p = L.GsMeshComponentsParams()
    p.faces, p.face_stride, p.n_faces, p.n_vertices = faces.data_ptr(), 3, m, n
    p.label, p.face_count, p.status = out.data_ptr(), out.data_ptr() + 4 * n, out.data_ptr() + 8 * n
    lib, stream = L.load(), _stream_ptr()
    hip = median_ms(lambda: L.check(lib.vmv_gs_mesh_components(C.byref(p), stream), "gs_mesh_components"), iters, warmup)
    label, count, status = out[:n].long(), out[n:2 * n].long(), int(out[2 * n])
    res = {}
    eager = median_ms(lambda: res.update(e=_components_eager(faces, n)), max(3, iters // 3), 1)
    drop = median_ms(lambda: res.update(d=drop_small_components(verts, cols, faces, min_fraction=0.05)), max(3, iters // 3), 1)
    sizes = count[count > 0].sort(descending=True).values
    r3 = lambda t: [round(x, 4) for x in t]
    return dict(mesh=name, vertices=n, faces=m, components=int((label == torch.arange(n, device="cuda")).sum()),
                largest_components=sizes[:6].tolist(), status=status, components_ms=r3(hip), eager_ms=r3(eager), drop_ms=r3(drop),
                ms_are="median, min, max", eager_over_hip=round(eager[0] / hip[0], 2),
                agrees_with_eager=bool(torch.equal(label, res["e"][0]) and torch.equal(count, res["e"][1])),
                dropped=res["d"][3])


def bake_record(name, verts, cols, faces, depth, colour, views, tan, voxel, patch, iters, warmup):
    """-> the JSON record of one mesh: the kernel and the torch restatement, and how far apart their textures are"""
    from videomv_amd import _lib as L
    from videomv_amd.gs_mesh import _bake_eager, texture_atlas
    from videomv_amd.ops import _stream_ptr
    n, m, V, S = int(verts.shape[0]), int(faces.shape[0]), int(depth.shape[0]), int(depth.shape[-1])
    asked = patch
    while patch > 4 and patch * (math.isqrt((m + 1) // 2 - 1) + 1) > 8192:      # the largest patch whose atlas fits a texture of 8192
        patch -= 1
    T, _ = texture_atlas(m, patch)
    verts, cols, faces = verts.contiguous(), cols.contiguous(), faces.contiguous()
    tex = torch.empty(4, T, T, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    tol = 2.0 * voxel
    p = L.GsMeshBakeParams()
    p.verts, p.vert_colours, p.faces, p.face_stride, p.n_faces, p.n_vertices = verts.data_ptr(), cols.data_ptr(), faces.data_ptr(), 3, m, n
    p.depth, p.colour, p.views, p.n_views, p.size, p.tan_half_fov = depth.data_ptr(), colour.data_ptr(), views.data_ptr(), V, S, tan
    p.z_min, p.depth_tol, p.cos_min, p.patch, p.tex_size = 0.05, tol, 0.1, patch, T
    p.out, p.plane_stride, p.status = tex.data_ptr(), T * T, status.data_ptr()
    lib, stream = L.load(), _stream_ptr()
    hip = median_ms(lambda: L.check(lib.vmv_gs_mesh_bake(C.byref(p), stream), "gs_mesh_bake"), iters, warmup)
    res = {}
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    eager = median_ms(lambda: res.update(e=_bake_eager(verts, cols, faces, depth, colour, views.reshape(V, 4, 4), f32(tan), patch, T, f32(tol), f32(0.1),
                                                       f32(0.05))), max(3, iters // 3), 1)
    ref = res["e"][0]
    owned = int((tex[3] >= 0).sum())
    r3 = lambda t: [round(x, 4) for x in t]
    diff = (tex[:3] - ref[:3]).abs().amax(0)[(tex[3] > 0) & (ref[3] > 0)]
    return dict(mesh=name, vertices=n, faces=m, views=V, size=S, patch=patch, patch_asked=asked, texture=T, texels_of_faces=owned,
                baked=round(int((tex[3] > 0).sum()) / max(owned, 1), 4), status=int(status), bake_ms=r3(hip), eager_ms=r3(eager),
                ms_are="median, min, max", eager_over_hip=round(eager[0] / hip[0], 2),
                texel_views_per_s=round(owned * V / (hip[0] * 1e-3), 0), plane_bytes_per_s=round(16.0 * T * T / (hip[0] * 1e-3), 0),
                map_bytes=int(depth.numel() * 4 + colour.numel() * 4),
                sets_that_differ_from_eager=round(float(((tex[3] > 0) != (ref[3] > 0)).float().mean()), 6),
                baked_rgb_beyond_1e4_of_eager=round(float((diff > 1e-4).float().mean()), 6), baked_rgb_median_diff_vs_eager=float(diff.median()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128:24:256,256:48:512", help="R:V:S, comma-separated")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=65536)
    ap.add_argument("--log", default=None)
    ap.add_argument("--components", action="store_true", help="measure the component labelling on the extracted meshes instead")
    ap.add_argument("--bake", action="store_true", help="measure the texture baking on the extracted meshes instead")
    ap.add_argument("--patch", type=int, default=8, help="--bake: texels per side of an atlas cell")
    args = ap.parse_args(argv)
    if (args.components or args.bake) and not args.log:
        args.log = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "gs_mesh_cc_bench.log" if args.components else "gs_mesh_bake_bench.log")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as fh:
                fh.write(line + "\n")
    from videomv_amd.gs_export import _unpremultiplied
    from videomv_amd.gs import GaussianRenderer
    from videomv_amd.gs_mesh import TsdfVolume, mesh_stats
    g = scene(args.gaussians, 1).cuda()
    for R, V, S in (tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")):
        cv, cvp = orbit(V)
        r = GaussianRenderer(S)
        out = r.render_depth(g.unsqueeze(0), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None, bg_color=torch.full((3,), 0.5).cuda())
        depth, colour = out["median_depth"][0, :, 0].contiguous(), _unpremultiplied(out, 0.5).contiguous()
        views = cv.cuda()
        half = 2.0 * math.sin(0.5 * math.radians(r.fovy))
        if args.components:
            vol = TsdfVolume(R, half)
            vol.integrate(depth, views, r.tan_half_fov, colour=colour)
            emit(components_record(f"extract R={R} V={V} S={S}", *vol.extract(), args.iters, args.warmup))
            continue
        if args.bake:
            vol = TsdfVolume(R, half)
            vol.integrate(depth, views, r.tan_half_fov, colour=colour)
            emit(bake_record(f"extract R={R} V={V} S={S}", *vol.extract(), depth, colour, views.reshape(V, 16).contiguous(), r.tan_half_fov, vol.voxel,
                             args.patch, args.iters, args.warmup))
            continue
        vol = TsdfVolume(R, half)
        hip = median_ms(lambda: vol.integrate(depth, views, r.tan_half_fov, colour=colour), args.iters, args.warmup)
        # one call each from zero: the mesh, and the eager formulation's planes against the kernel's
        vol = TsdfVolume(R, half)
        vol.integrate(depth, views, r.tan_half_fov, colour=colour)
        res = {}
        ext = median_ms(lambda: res.update(m=vol.extract()), 5, 1)
        verts, _, faces = res["m"]
        st = mesh_stats(verts, faces)
        geo = ([float(torch.tensor(o, dtype=torch.float32)) for o in vol.origin], vol.voxel, vol.trunc)
        vlist = [[float(x) for x in m.reshape(-1)] for m in cv]
        acc = torch.zeros_like(vol.acc)
        eager = median_ms(lambda: eager_integrate(acc, depth, colour, vlist, r.tan_half_fov, *geo, 0.05, True), max(3, args.iters // 3), 1)
        acc.zero_()
        eager_integrate(acc, depth, colour, vlist, r.tan_half_fov, *geo, 0.05, True)
        torch.cuda.synchronize()
        differ = float((acc[[1, 2, 6]] != vol.acc[[1, 2, 6]]).float().mean())
        n, r3 = R ** 3, lambda t: [round(x, 4) for x in t]
        emit(dict(res=R, views=V, size=S, gaussians=args.gaussians, pixels_with_depth=round(float((depth > 0).float().mean()), 4),
                  integrate_ms=r3(hip), eager_ms=r3(eager), ms_are="median, min, max", eager_over_hip=round(eager[0] / hip[0], 2),
                  depth_gathers_per_s=round(n * V / (hip[0] * 1e-3), 0), plane_bytes_per_s=round(7 * n * 4 * 2 / (hip[0] * 1e-3), 0),
                  map_bytes=int(depth.numel() * 4 + colour.numel() * 4), plane_bytes=7 * n * 4 * 2,
                  extract_ms=r3(ext), mesh=dict(vertices=st["vertices"], faces=st["faces"], open_edges=st["open_edges"], euler=st["euler"]),
                  counts_that_differ_from_eager=differ, tsdf_max_diff_vs_eager=float((acc[0] - vol.acc[0]).abs().max())))
    if args.components:
        T = 65536
        i = torch.arange(T)
        strip = torch.randperm(T + 2, generator=torch.Generator().manual_seed(11))[torch.stack([i, i + 1, i + 2], dim=1)].cuda()
        v = torch.zeros(T + 2, 3, device="cuda")
        emit(components_record("strip of 65536 triangles, permuted numbering", v, v, strip, args.iters, args.warmup))


if __name__ == "__main__":
    main()
