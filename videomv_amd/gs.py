"""``GaussianRenderer`` — the LGM branch's splatting renderer on the gfx950 rasteriser (``csrc/raster.hip``).

Mirrors ``core/gs.py:16-94`` of the reference: ``render(gaussians [B,N,14], cam_view, cam_view_proj, cam_pos, bg_color)``
-> ``{"image": [B,V,3,S,S] (clamped to [0,1]), "alpha": [B,V,1,S,S]}``.  The reference rasterises one (sample, view) at a time;
here ALL B * V views of a call go through ONE batched pass (``vmv_gs_batch_*``: one preprocess launch, one scan, one radix sort with
the view in the key, one blend launch over tiles x views) and the host reads the instance total ONCE per call — 48 host round trips
per LGM-refined step in round 4, one now (``VMV_GS_BATCH=0`` restores the per-view loop; both share their device code and give the
same bits).  The reference delegates to the third-party ``diff_gaussian_rasterization`` extension, which is absent and unpinned; the
kernels follow the published forward algorithm (oracle/gs_ref.py, parity unpinned — DESIGN.md §2).
``render_depth`` is the same batched pass with the blend's depth mode (the extension's ``rendered_depth`` and a median depth per pixel);
``depth_to_points`` / ``merge_points_voxel`` / ``save_points_ply`` turn its maps into a coloured point cloud.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .ops import _stream_ptr


def depth_to_points(depth, cam_view, tan_half_fov, mask=None):
    """Unproject one depth map [S, S] (view depth z per pixel, 0 = nothing) to world points with the rasteriser's pixel convention:
    a Gaussian's centre lands on px = ((ndc + 1) S - 1) / 2 at INTEGER pixel coordinates, so pixel px looks along
    ndc = (2 px + 1) / S - 1 and x_view = z tan ndc_x (likewise y); then [x, y, z, 1] @ inverse(cam_view) (row-vector convention).
    Keeps the pixels with depth > 0 (and ``mask``, if given).  -> (points [n, 3], flat indices [n] of the pixels kept, row-major)."""
    S = depth.shape[-1]
    z = depth.reshape(S, S).to(torch.float32)
    keep = z > 0
    if mask is not None:
        keep = keep & mask.reshape(S, S).to(keep.device)
    idx = torch.nonzero(keep.reshape(-1)).flatten()
    zk = z.reshape(-1)[idx]
    ndc_x = (2.0 * (idx % S).to(torch.float32) + 1.0) / S - 1.0
    ndc_y = (2.0 * torch.div(idx, S, rounding_mode="floor").to(torch.float32) + 1.0) / S - 1.0
    pv = torch.stack([zk * tan_half_fov * ndc_x, zk * tan_half_fov * ndc_y, zk, torch.ones_like(zk)], dim=1)
    c2w = torch.inverse(cam_view.to(torch.float32).cpu()).to(z.device)
    return (pv @ c2w)[:, :3], idx


def merge_points_voxel(points, colours, voxel):
    """One point per occupied cube of side ``voxel``: the mean position and the mean colour of the points inside (no RNG, order of
    torch.unique).  points [n, 3], colours [n, 3] -> ([m, 3], [m, 3])."""
    q = torch.floor(points / voxel).to(torch.int64)
    _, inv, counts = torch.unique(q, dim=0, return_inverse=True, return_counts=True)
    m = counts.shape[0]
    both = torch.zeros(m, 6, dtype=torch.float32, device=points.device)
    both.index_add_(0, inv, torch.cat([points.float(), colours.float()], dim=1))
    both = both / counts.to(torch.float32).unsqueeze(1)
    return both[:, :3], both[:, 3:]


def save_points_ply(points, colours, path):
    """points [n, 3] fp32, colours [n, 3] in [0, 1] -> binary little-endian .ply: x y z float32, red green blue uchar (rounded).
    Returns the number of vertices written."""
    n = int(points.shape[0])
    rows = np.empty(n, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    rows["xyz"] = points.detach().float().cpu().numpy()
    rows["rgb"] = (colours.detach().float().cpu().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).numpy()
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join("property float %s\n" % a for a in "xyz") + "".join("property uchar %s\n" % a for a in ("red", "green", "blue"))
    with open(path, "wb") as f:
        f.write((header + "end_header\n").encode("ascii"))
        f.write(rows.tobytes())
    return n


def load_points_ply(path):
    """The inverse of ``save_points_ply`` -> (points [n, 3] fp32, colours [n, 3] uint8)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or props != [["float", a] for a in "xyz"] + [["uchar", a] for a in ("red", "green", "blue")]:
        raise ValueError(f"{path}: not a point cloud written by save_points_ply")
    n = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    rows = np.frombuffer(data, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)], count=n, offset=end)
    return torch.from_numpy(rows["xyz"].copy()), torch.from_numpy(rows["rgb"].copy())


class GaussianRenderer:
    def __init__(self, output_size=512, fovy=39.6, znear=0.5, zfar=2.5):
        self.size, self.fovy = int(output_size), float(fovy)
        self.tan_half_fov = math.tan(0.5 * math.radians(self.fovy))
        self.proj_matrix = torch.zeros(4, 4, dtype=torch.float32)          # core/gs.py:23-29
        self.proj_matrix[0, 0] = 1 / self.tan_half_fov
        self.proj_matrix[1, 1] = 1 / self.tan_half_fov
        self.proj_matrix[2, 2] = (zfar + znear) / (zfar - znear)
        self.proj_matrix[3, 2] = -(zfar * znear) / (zfar - znear)
        self.proj_matrix[2, 3] = 1
        self._buf = {}
        self.last_num_rendered, self.last_views = [], 0

    def _buffers(self, N, device):
        key = (N, str(device))
        b = self._buf.get(key)
        if b is None:
            lib = L.load()
            sb, so = C.c_size_t(0), C.c_size_t(0)
            L.check(lib.vmv_gs_workspace_bytes(N, 1, C.byref(sb), C.byref(so)), "gs_workspace_bytes")
            grid = (self.size + 15) // 16
            f = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=device)
            b = dict(depth=f(N), xy=f(N, 2), co=f(N, 4), rect=f(N, 4, dt=torch.int32), touched=f(N, dt=torch.int32),
                     offsets=f(N, dt=torch.int32), scan=torch.zeros(max(int(sb.value), 16), dtype=torch.uint8, device=device),
                     ranges=f(grid * grid, 2, dt=torch.int32), cap=0)
            self._buf[key] = b
        return b

    @staticmethod
    def _attach_instances(p, buf, n, device, workspace_bytes):
        """The binning buffers of ``n`` instances for the pass ``p`` (GsParams or GsBatchParams), shared by the per-view and the batched
        path: grows the key / value / sort buffers of ``buf`` with 1.25 head-room (``workspace_bytes(cap, scan_ref, sort_ref)`` = the
        path's own workspace-size call) and attaches them, the count and the ranges to ``p``."""
        if n > buf["cap"]:
            cap = max(int(n * 1.25), 1 << 16)
            sb, so = C.c_size_t(0), C.c_size_t(0)
            L.check(workspace_bytes(cap, C.byref(sb), C.byref(so)), "gs_workspace_bytes")
            i64 = lambda: torch.zeros(cap, dtype=torch.int64, device=device)
            i32 = lambda: torch.zeros(cap, dtype=torch.int32, device=device)
            buf.update(keys=i64(), keys_s=i64(), vals=i32(), vals_s=i32(), cap=cap,
                       sort=torch.zeros(max(int(so.value), 16), dtype=torch.uint8, device=device))
        p.num_rendered = buf["n"] = n
        if n > 0:
            p.keys, p.keys_sorted, p.vals, p.vals_sorted = (buf["keys"].data_ptr(), buf["keys_s"].data_ptr(), buf["vals"].data_ptr(),
                                                            buf["vals_s"].data_ptr())
            p.sort_temp, p.sort_temp_bytes = buf["sort"].data_ptr(), buf["sort"].numel()
        p.ranges = buf["ranges"].data_ptr()

    @staticmethod
    def _attach_preprocess(p, buf):
        """the per-Gaussian arrays and the scan workspace of ``buf`` for the pass ``p`` (GsParams or GsBatchParams)"""
        p.depth, p.xy, p.conic_opacity, p.rect = buf["depth"].data_ptr(), buf["xy"].data_ptr(), buf["co"].data_ptr(), buf["rect"].data_ptr()
        p.tiles_touched, p.offsets = buf["touched"].data_ptr(), buf["offsets"].data_ptr()
        p.scan_temp, p.scan_temp_bytes = buf["scan"].data_ptr(), buf["scan"].numel()

    def _batch_buffers(self, B, V, N, device):
        key = ("batch", B, V, N, str(device))
        b = self._buf.get(key)
        if b is None:
            lib = L.load()
            VN = B * V * N
            bits = lib.vmv_gs_batch_key_bits(B * V, self.size)
            sb, so = C.c_size_t(0), C.c_size_t(0)
            L.check(lib.vmv_gs_batch_workspace_bytes(VN, 1, bits, C.byref(sb), C.byref(so)), "gs_batch_workspace_bytes")
            grid = (self.size + 15) // 16
            f = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=device)
            b = dict(depth=f(VN), xy=f(VN, 2), co=f(VN, 4), rect=f(VN, 4, dt=torch.int32), touched=f(VN, dt=torch.int32),
                     offsets=f(VN, dt=torch.int32), scan=torch.zeros(max(int(sb.value), 16), dtype=torch.uint8, device=device),
                     ranges=f(B * V * grid * grid, 2, dt=torch.int32), cap=0, bits=bits,
                     total=torch.zeros(1, dtype=torch.int32).pin_memory() if str(device).startswith("cuda") else torch.zeros(1, dtype=torch.int32))
            self._buf[key] = b
        return b

    @staticmethod
    def _stage_arrays(buf, shape, n, key_dtype):
        """views (no copy, no device work) of what the last pass over ``buf`` left on the device; ``shape`` = the leading dimensions of the
        per-Gaussian arrays, ``key_dtype`` = the form of key that pass sorted (they are the first n entries of the key buffer)"""
        empty = lambda dt: torch.empty(0, dtype=dt, device=buf["depth"].device)
        has = n > 0 and "keys_s" in buf
        return dict(n=n, depth=buf["depth"].view(*shape), xy=buf["xy"].view(*shape, 2), conic_opacity=buf["co"].view(*shape, 4),
                    rect=buf["rect"].view(*shape, 4), tiles_touched=buf["touched"].view(*shape), offsets=buf["offsets"].view(*shape),
                    ranges=buf["ranges"].view(*shape[:-1], -1, 2),
                    keys_sorted=buf["keys_s"].view(key_dtype)[:n] if has else empty(key_dtype),
                    vals_sorted=buf["vals_s"][:n] if has else empty(torch.int32))

    def binning(self, B, V, N, device):
        """The intermediate arrays of the last BATCHED pass at this shape (``render``, ``render_depth``, GaussianFitter's forward), read
        only: n (the instance total), depth / tiles_touched / offsets [B * V, N], xy [B * V, N, 2], conic_opacity [B * V, N, 4],
        rect [B * V, N, 4] (records with tiles_touched == 0 keep whatever they held), ranges [B * V, tiles, 2], and the first n sorted
        (view, tile) keys (int32) and values (the Gaussian's index in its sample).  ``offsets`` are in depth-rank order."""
        buf = self._buf[("batch", B, V, N, str(device))]
        return self._stage_arrays(buf, (B * V, N), buf.get("n", 0), torch.int32)

    def binning_view(self, N, device):
        """``binning`` for the per-view path (VMV_GS_BATCH=0): the arrays of the LAST view rendered, leading dimension 1, the keys in
        that path's form (int64: tile << 32 | depth bits), ``offsets`` in index order."""
        buf = self._buf[(N, str(device))]
        return self._stage_arrays(buf, (1, N), buf.get("n", 0), torch.int64)

    def _batch_setup(self, p, gaussians, views, view_projs, B, V, N, bg, limit):
        """Everything of one batched pass before its blend, for the renderer and for GaussianFitter: fills ``p`` (GsBatchParams) from
        contiguous fp32 device tensors (gaussians [B, N, 14], views / view_projs [B * V, 16]), runs the preprocess, reads the instance
        total, and sizes and attaches the binning buffers.  -> (n, ok): the total, and whether it is within ``limit``; nothing is
        attached when it is not."""
        device = gaussians.device
        lib = L.load()
        buf = self._batch_buffers(B, V, N, device)
        p.gaussians, p.B, p.N, p.V, p.size = gaussians.data_ptr(), B, N, V, self.size
        p.views, p.view_projs, p.tan_half_fov = views.data_ptr(), view_projs.data_ptr(), self.tan_half_fov
        p.bg[0], p.bg[1], p.bg[2] = bg
        self._attach_preprocess(p, buf)
        L.check(lib.vmv_gs_batch_preprocess(C.byref(p), _stream_ptr()), "gs_batch_preprocess")
        # the ONE host round trip of the call: the instance total sizes the sort (pinned destination: a 4-byte copy + stream sync)
        buf["total"].copy_(buf["offsets"][B * V * N - 1:], non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
        n = int(buf["total"][0])
        # The scan and `num_rendered` are int32.  The caller bounds B * V * N * tiles below 2^32, so a total past 2^31 - 1 shows up as a
        # NEGATIVE count (never as a small positive one): refuse it, and refuse totals whose key / value buffers (24 B per instance,
        # x 1.25 head-room) would pass the caller's budget.
        if n < 0 or n > limit:
            return n, False
        self._attach_instances(p, buf, n, device, lambda cap, sb, so: lib.vmv_gs_batch_workspace_bytes(B * V * N, cap, buf["bits"], sb, so))
        return n, True

    def _render_batch(self, gaussians, cam_view, cam_view_proj, bg, images, alphas, depths=None, medians=None):
        """All B * V views in one pass (vmv.h VmvGsBatchParams); with ``depths`` / ``medians`` the blend is the depth mode's
        (VmvGsDepthParams: the same pass, the same image and alpha bits).  -> False when the instance total passes
        ``max_batch_instances``: the caller then splits the views."""
        device = gaussians.device
        B, V = cam_view.shape[:2]
        lib = L.load()
        g = gaussians.float().contiguous()
        views = cam_view.to(device, torch.float32).reshape(B * V, 16).contiguous()
        vps = cam_view_proj.to(device, torch.float32).reshape(B * V, 16).contiguous()
        dp = L.GsDepthParams()
        p = dp.pass_
        n, ok = self._batch_setup(p, g, views, vps, B, V, gaussians.shape[1], bg, self.max_batch_instances)
        if not ok:
            return False
        self.last_num_rendered.append(n)
        p.out_color, p.out_alpha = images.data_ptr(), alphas.data_ptr()
        if depths is None:
            L.check(lib.vmv_gs_batch_render(C.byref(p), _stream_ptr()), "gs_batch_render")
        else:
            dp.out_depth, dp.out_median_depth = depths.data_ptr(), None if medians is None else medians.data_ptr()
            L.check(lib.vmv_gs_batch_render_depth(C.byref(dp), _stream_ptr()), "gs_batch_render_depth")
        self._keep.append((g, views, vps))    # (referenced by the enqueued launches)
        return True

    def _render_views(self, gaussians, cam_view, cam_view_proj, bg, *outs):
        """The batched pass over as many views at a time as its 32-bit instance count and the memory budget allow: all B * V at once when
        they fit (the VideoMV shapes: 2 x 24 views, 21 M instances), else per sample, else halves of a sample's views; a single view that
        still does not fit goes to the per-view entry points.  Chunks are independent renders: images are those of the one-pass call.
        ``outs`` = the [B, V, ...] output tensors of ``_render_batch`` (images, alphas and, in the depth mode, depths, medians)."""
        B, V = cam_view.shape[:2]
        N, tiles = gaussians.shape[1], ((self.size + 15) // 16) ** 2
        if B * V * N * tiles < (1 << 32) and B * V * N < (1 << 31) and B * V <= 65535:
            if self._render_batch(gaussians, cam_view, cam_view_proj, bg, *outs):
                return True
        if B > 1:
            return all(self._render_views(gaussians[b:b + 1], cam_view[b:b + 1], cam_view_proj[b:b + 1], bg, *(o[b:b + 1] for o in outs))
                       for b in range(B))
        if V > 1:
            h = V // 2
            return all(self._render_views(gaussians, cam_view[:, a:z], cam_view_proj[:, a:z], bg, *(o[:, a:z] for o in outs))
                       for a, z in ((0, h), (h, V)))
        return False

    def _begin(self, gaussians, cam_view, bg_color, planes):
        """Common start of ``render`` / ``render_depth``: the background, one empty [B, V, c, S, S] fp32 output per entry of ``planes``,
        the per-call records and the instance budget."""
        import os
        B, V = cam_view.shape[:2]
        bg = [1.0, 1.0, 1.0] if bg_color is None else [float(v) for v in bg_color.reshape(-1)[:3]]
        outs = [torch.empty(B, V, c, self.size, self.size, dtype=torch.float32, device=gaussians.device) for c in planes]
        self.last_num_rendered, self.last_views, self._keep = [], B * V, []
        self.max_batch_instances = min((1 << 31) - 1, int(os.environ.get("VMV_GS_BATCH_MAX_INSTANCES", str(1 << 28))))   # 2^28 x 30 B = 8 GB
        return bg, outs

    @torch.no_grad()
    def render_depth(self, gaussians, cam_view, cam_view_proj, cam_pos=None, bg_color=None):
        """``render`` plus geometry, through the batched pass's depth mode (vmv_gs_batch_render_depth; chunked like ``render``):
        -> ``{"image", "alpha"}`` with ``render``'s bits, ``"depth"`` [B,V,1,S,S] = sum alpha T z over the blended Gaussians (view depth,
        not normalised: the extension's ``rendered_depth``) and ``"median_depth"`` [B,V,1,S,S] = z of the first blended Gaussian after
        which the transmittance is below 0.5, 0 where it never is.  The per-view entry points have no depth mode: a single view whose
        instances pass VMV_GS_BATCH_MAX_INSTANCES is refused."""
        bg, outs = self._begin(gaussians, cam_view, bg_color, (3, 1, 1, 1))
        if not self._render_views(gaussians, cam_view, cam_view_proj, bg, *outs):
            raise NotImplementedError("render_depth: a single view does not fit the batched pass (VMV_GS_BATCH_MAX_INSTANCES = "
                                      f"{self.max_batch_instances}) and the per-view entry points have no depth mode")
        return dict(zip(("image", "alpha", "depth", "median_depth"), outs))

    @torch.no_grad()
    def render(self, gaussians, cam_view, cam_view_proj, cam_pos=None, bg_color=None, scale_modifier=1):
        if scale_modifier != 1:
            raise NotImplementedError("scale_modifier != 1 is not a VideoMV configuration")
        import os
        device = gaussians.device
        B, V = cam_view.shape[:2]
        N, S = gaussians.shape[1], self.size
        lib = L.load()
        bg, (images, alphas) = self._begin(gaussians, cam_view, bg_color, (3, 1))
        if os.environ.get("VMV_GS_BATCH", "1") != "0":
            if self._render_views(gaussians, cam_view, cam_view_proj, bg, images, alphas):
                return {"image": images, "alpha": alphas}
        buf = self._buffers(N, device)
        self.last_num_rendered = []           # (drops the chunks a batched attempt rendered before one view was refused)
        workspace_bytes = lambda cap, sb, so: lib.vmv_gs_workspace_bytes(N, cap, sb, so)
        for b in range(B):
            g = gaussians[b].float().contiguous()
            for v in range(V):
                view = cam_view[b, v].float().contiguous().to(device)
                vp = cam_view_proj[b, v].float().contiguous().to(device)
                p = L.GsParams()
                p.gaussians, p.N, p.size, p.view, p.view_proj = g.data_ptr(), N, S, view.data_ptr(), vp.data_ptr()
                p.tan_half_fov = self.tan_half_fov
                p.bg[0], p.bg[1], p.bg[2] = bg
                self._attach_preprocess(p, buf)
                L.check(lib.vmv_gs_preprocess(C.byref(p), _stream_ptr()), "gs_preprocess")
                n = int(buf["offsets"][N - 1].item())                       # the one host round trip per view
                self.last_num_rendered.append(n)
                self._attach_instances(p, buf, n, device, workspace_bytes)
                p.out_color, p.out_alpha = images[b, v].data_ptr(), alphas[b, v].data_ptr()
                L.check(lib.vmv_gs_render(C.byref(p), _stream_ptr()), "gs_render")
        return {"image": images, "alpha": alphas}

    # ------------------------------------------------------------------ .ply export (core/gs.py:97-186 of the reference)
    PLY_PROPERTIES = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
                      "rot_0", "rot_1", "rot_2", "rot_3")

    def save_ply(self, gaussians, path, compatible=True):
        """gaussians [1, N, 14] (activated: pos, opacity, scale, rotation, rgb) -> binary little-endian .ply of the 3-D Gaussian
        Splatting layout, rows with opacity < 0.005 dropped; ``compatible`` stores the pre-activation values (logit opacity, log
        scale, SH-DC colour).  Written by hand (the reference uses plyfile).  Returns the number of vertices written."""
        assert gaussians.shape[0] == 1, 'only support batch size 1'
        g = gaussians[0].detach().float().cpu()
        g = g[g[:, 3] >= 0.005]
        pos, opacity, scales, rots, rgb = g[:, 0:3], g[:, 3:4], g[:, 4:7], g[:, 7:11], g[:, 11:14]
        if compatible:
            o = opacity.clamp(1e-6, 1 - 1e-6)                        # kiui.op.inverse_sigmoid
            opacity = torch.log(o / (1 - o))
            scales = torch.log(scales + 1e-8)
            rgb = (rgb - 0.5) / 0.28209479177387814
        body = torch.cat([pos, rgb, opacity, scales, rots], dim=1).numpy().astype("<f4")
        header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % body.shape[0]
        header += "".join("property float %s\n" % n for n in self.PLY_PROPERTIES) + "end_header\n"
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(np.ascontiguousarray(body).tobytes())
        return int(body.shape[0])

    @classmethod
    def load_ply(cls, path, compatible=True):
        """The inverse of ``save_ply`` (any binary little-endian vertex element with float properties that include the 14 names):
        -> gaussians [N, 14] activated (fp32, CPU)."""
        with open(path, "rb") as f:
            data = f.read()
        end = data.index(b"end_header\n") + len(b"end_header\n")
        lines = data[:end].decode("ascii").splitlines()
        if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
            raise ValueError(f"{path}: not a binary little-endian .ply")
        count, names = None, []
        for ln in lines[2:]:
            w = ln.split()
            if w[0] == "element":
                if count is not None:
                    break                                              # (only the first element, the vertices, is read)
                count = int(w[2])
            elif w[0] == "property":
                if w[1] != "float":
                    raise ValueError(f"{path}: property {ln!r} is not a float")
                names.append(w[2])
        rows = np.frombuffer(data, dtype="<f4", count=count * len(names), offset=end).reshape(count, len(names))
        col = {n: rows[:, i] for i, n in enumerate(names)}
        order = ("x", "y", "z", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "f_dc_0", "f_dc_1", "f_dc_2")
        g = torch.from_numpy(np.stack([col[n] for n in order], axis=1).astype(np.float32))
        if compatible:
            g[:, 3:4] = torch.sigmoid(g[:, 3:4])
            g[:, 4:7] = torch.exp(g[:, 4:7])
            g[:, 11:] = 0.28209479177387814 * g[:, 11:] + 0.5
        return g
