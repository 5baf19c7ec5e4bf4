"""A coloured triangle mesh from depth maps: TSDF fusion on the gfx950 kernel (``csrc/gs_tsdf.hip``, contract in ``include/vmv.h``)
and naive surface nets over the fused field, in vectorised torch on the device the accumulators live on.

``TsdfVolume`` owns the seven accumulator planes of ``VmvGsTsdfParams`` and turns them into a signed field; ``surface_nets`` places one
vertex per sign-changing cell and one quad per sign-changing grid edge; ``mesh_stats`` counts what a consumer would trip over (open and
misoriented edges, the Euler characteristic, the signed volume); ``mesh_components`` labels the connected components of a mesh
(``csrc/gs_mesh_cc.hip`` on the device, a torch propagation on the CPU) and ``drop_small_components`` removes the floaters among them;
``save_mesh_ply`` / ``load_mesh_ply`` are the binary little-endian writer and its inverse; ``texture_atlas`` lays two faces into every
P x P cell of a square texture, ``bake_texture`` blends the depth-mapped views over the surface into it (``csrc/gs_mesh_bake.hip`` on the
device, a torch restatement on the CPU) and ``save_mesh_obj`` / ``load_mesh_obj`` write and read the textured .obj.  No RNG anywhere:
the same inputs give the same file.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L

PLANES = ("tsdf", "weight", "behind", "red", "green", "blue", "colour_weight")


def _view_tensors(depth, colour, cam_view, dev):
    """The views as the kernels read them: contiguous fp32 depth [V, S, S], colour [V, 3, S, S] (or None) and cameras [V, 16] on ``dev``."""
    V, S = int(depth.shape[0]), int(depth.shape[-1])
    d, col, views = depth.reshape(V, S, S), None if colour is None else colour.reshape(V, 3, S, S), cam_view.reshape(V, 16)
    return tuple(t if t is None else t.to(dev, torch.float32).contiguous() for t in (d, col, views))


def _kernel_faces(faces):
    """``faces`` as the kernels read them: the three indices of a face adjacent, a face stride >= 3"""
    return faces if faces.stride(1) == 1 and faces.stride(0) >= 3 else faces.contiguous()


def _raise_status(status, what, n):
    """The status word of vmv_gs_mesh_components / vmv_gs_mesh_bake (bits: _lib.MESH_STATUS_*), or of a CPU path, as its exception."""
    if status & L.MESH_STATUS_GAVE_UP:
        raise RuntimeError(f"{what}: a bounded loop of the union-find gave up (status bit 1): the label buffer was written during the call")
    if status & L.MESH_STATUS_RANGE:
        raise ValueError(f"{what}: a face names a vertex outside [0, {n})")


class TsdfVolume:
    """res^3 voxel CENTRES over the cube centre +- half_extent: voxel = 2 half_extent / res, centre i at origin + i * voxel with
    origin = centre - half_extent + voxel / 2.  ``acc`` [7, res, res, res] (planes of VmvGsTsdfParams, [z][y][x]) starts at zero."""

    def __init__(self, res, half_extent, centre=(0.0, 0.0, 0.0), trunc=None, device="cuda"):
        self.res = int(res)
        self.voxel = 2.0 * float(half_extent) / self.res
        self.origin = tuple(float(c) - float(half_extent) + 0.5 * self.voxel for c in centre)
        self.trunc = 3.0 * self.voxel if trunc is None else float(trunc)
        self.acc = torch.zeros(7, self.res, self.res, self.res, dtype=torch.float32, device=device)
        self.n_views = 0

    @torch.no_grad()
    def integrate(self, depth, cam_view, tan_half_fov, colour=None, carve=True, z_min=0.05):
        """Fuse ``depth`` [V, S, S] (view depth per pixel, 0 = no surface) seen through ``cam_view`` [V, 4, 4] (row-vector convention),
        with ``colour`` [V, 3, S, S] if given, into the volume: one launch of vmv_gs_tsdf_integrate on the current stream."""
        from .ops import _stream_ptr
        dev = self.acc.device
        if dev.type != "cuda":
            raise RuntimeError("TsdfVolume.integrate runs the HIP kernel: the volume must live on a GPU (there is no CPU fallback)")
        d, col, views = _view_tensors(depth, colour, cam_view, dev)
        V, S = d.shape[:2]
        p = L.GsTsdfParams()
        p.depth, p.colour, p.views = d.data_ptr(), None if col is None else col.data_ptr(), views.data_ptr()
        p.n_views, p.size, p.tan_half_fov, p.res = V, S, float(tan_half_fov), self.res
        p.origin[0], p.origin[1], p.origin[2] = self.origin
        p.voxel, p.trunc, p.z_min, p.carve = self.voxel, self.trunc, float(z_min), 1 if carve else 0
        p.acc, p.plane_stride = self.acc.data_ptr(), self.res ** 3
        L.check(L.load().vmv_gs_tsdf_integrate(C.byref(p), _stream_ptr()), "gs_tsdf_integrate")
        self.n_views += V

    def field(self, min_weight=1):
        """-> (f, valid) [res, res, res]: f = sum tsdf / W where W >= min_weight; f = -1 where the voxel was never in front of or near a
        surface (W == 0) and hidden behind one in EVERY view integrated (n_behind == n_views): solid; every other voxel is invalid
        (f = 0 there).  "Every", not "any": a voxel that leaves some view's frustum is not known to be solid."""
        tsdf, w, behind = self.acc[0], self.acc[1], self.acc[2]
        seen = w >= float(min_weight)
        solid = (w == 0) & (behind == float(self.n_views)) & (self.n_views > 0)
        f = torch.where(seen, tsdf / w.clamp_min(1.0), torch.where(solid, -torch.ones_like(w), torch.zeros_like(w)))
        return f, seen | solid

    def colours(self):
        """-> [3, res, res, res]: sum RGB / Wc, 0.5 where Wc == 0"""
        wc = self.acc[6]
        return torch.where(wc > 0, self.acc[3:6] / wc.clamp_min(1.0), torch.full_like(self.acc[3:6], 0.5))

    def extract(self, min_weight=1):
        """-> (verts [n, 3] fp32, colours [n, 3], faces [m, 3] int64) on the volume's device"""
        f, valid = self.field(min_weight)
        return surface_nets(f, valid, self.origin, self.voxel, colour=self.colours(), colour_weight=self.acc[6])


# the 8 corners of a cell as (dz, dy, dx), corner c = 4 dz + 2 dy + dx, and its 12 edges (corner pairs that differ in one bit)
_CORNERS = [(c >> 2 & 1, c >> 1 & 1, c & 1) for c in range(8)]
_EDGES = [(a, a | b) for a in range(8) for b in (1, 2, 4) if not a & b]
# grid edges along tensor dim a; (u, v) are the two other dims with e_a = e_u x e_v in the right-handed (x, y, z) = dims (2, 1, 0)
_AXES = ((2, 1, 0), (1, 0, 2), (0, 2, 1))


@torch.no_grad()
def surface_nets(f, valid, origin, voxel, colour=None, colour_weight=None):
    """Naive surface nets over the field ``f`` [R, R, R] ([z][y][x]; negative inside) at voxel centres origin + i * voxel.
    A cell (the cube between 8 neighbouring centres) is active if all 8 corners are ``valid`` and the signs of f < 0 are mixed; its
    vertex is the mean of the linear zero crossings t = f0 / (f0 - f1) on its sign-changing edges, its colour the ``colour_weight``-
    weighted mean of the 8 corner colours (``colour`` [3, R, R, R]; the plain mean where the weights sum to 0; 0.5 without ``colour``).
    Every grid edge whose ends differ in sign and whose four surrounding cells are all active emits the quad of their vertices as two
    triangles, wound so that the normal points from f < 0 to f > 0.  Vertices that no triangle uses are dropped.  Order: cells and
    edges row-major, x edges, then y, then z.  Runs on f's device.  -> (verts [n, 3] fp32 (x, y, z), colours [n, 3], faces [m, 3] int64)."""
    R, dev = int(f.shape[0]), f.device
    assert tuple(f.shape) == (R, R, R) and tuple(valid.shape) == (R, R, R) and R >= 2
    f = f.to(torch.float32)
    inside = f < 0
    n = R - 1
    cell = lambda t, c: t[c[0]:c[0] + n, c[1]:c[1] + n, c[2]:c[2] + n]
    n_in = torch.zeros(n, n, n, dtype=torch.int8, device=dev)
    ok = torch.ones(n, n, n, dtype=torch.bool, device=dev)
    for c in _CORNERS:
        n_in += cell(inside, c).to(torch.int8)
        ok &= cell(valid, c)
    active = ok & (n_in > 0) & (n_in < 8)
    zyx = active.nonzero()                                              # [k, 3] row-major
    k = int(zyx.shape[0])
    cid = torch.full((n, n, n), -1, dtype=torch.int64, device=dev)
    cid[active] = torch.arange(k, device=dev)
    # corner values of the active cells, by flat index into [R, R, R]
    offs = torch.tensor([(dz * R + dy) * R + dx for dz, dy, dx in _CORNERS], device=dev)
    idx8 = ((zyx[:, 0] * R + zyx[:, 1]) * R + zyx[:, 2])[:, None] + offs[None, :]          # [k, 8]
    fc = f.reshape(-1)[idx8]
    ea, eb = (torch.tensor([e[i] for e in _EDGES], device=dev) for i in (0, 1))
    fa, fb = fc[:, ea], fc[:, eb]
    cross = (fa < 0) != (fb < 0)
    t = torch.where(cross, fa / torch.where(cross, fa - fb, torch.ones_like(fa)), torch.zeros_like(fa))
    cp = torch.tensor([[dx, dy, dz] for dz, dy, dx in _CORNERS], dtype=torch.float32, device=dev)     # (x, y, z)
    pts = cp[ea][None] + t[..., None] * (cp[eb] - cp[ea])[None]                                        # [k, 12, 3]
    w = cross.to(torch.float32)
    local = (pts * w[..., None]).sum(1) / w.sum(1, keepdim=True).clamp_min(1.0)
    verts = torch.tensor(list(origin), dtype=torch.float32, device=dev) + (zyx.flip(1).to(torch.float32) + local) * float(voxel)
    if colour is None:
        cols = torch.full((k, 3), 0.5, dtype=torch.float32, device=dev)
    else:
        cc = colour.to(torch.float32).reshape(3, -1)[:, idx8]                                          # [3, k, 8]
        cw = torch.ones_like(fc) if colour_weight is None else colour_weight.to(torch.float32).reshape(-1)[idx8]
        ws = cw.sum(1)
        cols = torch.where(ws > 0, (cc * cw).sum(2) / ws.clamp_min(1e-20), cc.mean(2)).t().contiguous()
    faces = []
    m = R - 2
    for a, u, v in _AXES:
        inner = lambda x: x.narrow(u, 1, m).narrow(v, 1, m)
        lo, hi = inner(inside.narrow(a, 0, n)), inner(inside.narrow(a, 1, n))
        quad = [cid.narrow(u, du, m).narrow(v, dv, m) for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1))]   # counter-clockwise seen from +a
        emit = lo != hi
        for q in quad:
            emit = emit & (q >= 0)
        q = torch.stack([c[emit] for c in quad], dim=1)                                                # [e, 4]
        q = torch.where(lo[emit][:, None], q, q[:, [0, 3, 2, 1]])                                      # inside at the low end: normal along +a
        faces.append(torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], dim=1).reshape(-1, 3))
    faces = torch.cat(faces)
    used = torch.unique(faces)                                          # sorted: the vertex order is kept
    remap = torch.full((k,), -1, dtype=torch.int64, device=dev)
    remap[used] = torch.arange(int(used.shape[0]), device=dev)
    return verts[used], cols[used], remap[faces]


def mesh_stats(verts, faces):
    """-> dict: vertices, edges (undirected), faces, euler = V - E + F, open_edges (undirected edges not in exactly two triangles),
    misoriented (directed edges that occur more than once: two neighbours wound against each other), volume (signed: positive for
    outward normals)."""
    v, f = verts.detach().cpu().double(), faces.detach().cpu().long()
    nv = max(int(v.shape[0]), 1)
    d = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, dc = torch.unique(d[:, 0] * nv + d[:, 1], return_counts=True)
    _, uc = torch.unique(d.min(1).values * nv + d.max(1).values, return_counts=True)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    E = int(uc.shape[0])
    return dict(vertices=int(v.shape[0]), edges=E, faces=int(f.shape[0]), euler=int(v.shape[0]) - E + int(f.shape[0]),
                open_edges=int((uc != 2).sum()), misoriented=int((dc > 1).sum()),
                volume=float((a * torch.linalg.cross(b, c)).sum() / 6.0))


def _components_eager(faces, n):
    """The contract of ``mesh_components`` in torch, on faces' device: every round gives each vertex of a face, and the vertex its label
    names, the smallest label of the face (scatter amin), then jumps label <- label[label] twice; repeated until a round changes nothing.
    A label always names a vertex of the same component and never exceeds its own index, so the fixed point — constant on every face,
    hence on every component — is the component's smallest index.  ``faces`` [m, 3] in range.  -> (label, face_count) [n] int64."""
    label = torch.arange(n, dtype=torch.int64, device=faces.device)
    flat = faces.reshape(-1)
    while flat.numel():
        low = label[faces].min(dim=1).values.repeat_interleave(3)
        new = label.scatter_reduce(0, flat, low, "amin").scatter_reduce(0, label[flat], low, "amin")
        new = new[new]
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    count = torch.zeros(n, dtype=torch.int64, device=faces.device)
    if flat.numel():
        count.index_add_(0, label[faces[:, 0]], torch.ones_like(faces[:, 0]))
    return label, count


@torch.no_grad()
def mesh_components(faces, n_vertices):
    """Connected components of the mesh ``faces`` [m, 3] (int64) over ``n_vertices`` vertices -> (label [n] int64, face_count [n] int64):
    label[v] is the smallest vertex index of v's component (a vertex in no face is its own), face_count[r] the number of faces of the
    component labelled r and 0 elsewhere (the contract of vmv_gs_mesh_components, include/vmv.h).  CUDA tensors run the kernel on the
    current stream; CPU tensors the torch propagation above.  A face index outside [0, n_vertices) raises ValueError."""
    n, m = int(n_vertices), int(faces.shape[0])
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64 and n >= 0
    if n == 0 or not faces.is_cuda:                                     # (the kernel takes n >= 1: no vertices, no launch)
        _raise_status(L.MESH_STATUS_RANGE if m and bool(((faces < 0) | (faces >= n)).any()) else 0, "mesh_components", n)
        return _components_eager(faces, n) if n else (torch.zeros(0, dtype=torch.int64, device=faces.device),) * 2
    from .ops import _stream_ptr
    faces = _kernel_faces(faces)
    out = torch.empty(2 * n + 1, dtype=torch.int32, device=faces.device)
    p = L.GsMeshComponentsParams()
    p.faces = faces.data_ptr() if m else out.data_ptr()                 # no face is read when there is none
    p.face_stride, p.n_faces, p.n_vertices = (int(faces.stride(0)) if m else 3), m, n
    p.label, p.face_count, p.status = out.data_ptr(), out.data_ptr() + 4 * n, out.data_ptr() + 8 * n
    L.check(L.load().vmv_gs_mesh_components(C.byref(p), _stream_ptr()), "gs_mesh_components")
    _raise_status(int(out[2 * n]), "mesh_components", n)
    return out[:n].long(), out[n:2 * n].long()


@torch.no_grad()
def drop_small_components(verts, colours, faces, min_fraction=0.0, min_faces=0):
    """Remove the small connected components (floaters) of a mesh.  A component is kept iff its face count is >= ``min_faces`` and
    >= ``min_fraction`` x the largest component's face count; kept vertices and kept faces keep their order, indices are remapped; with
    both thresholds 0 everything is kept.  Runs on the tensors' device, draws no RNG.
    -> (verts, colours, faces, info) with info = dict(components, kept, largest_faces, dropped_faces, dropped_vertices)."""
    n, m = int(verts.shape[0]), int(faces.shape[0])
    label, count = mesh_components(faces, n)
    is_root = label == torch.arange(n, dtype=torch.int64, device=label.device)
    largest = int(count.max()) if n else 0
    keep_root = is_root & (count >= int(min_faces)) & (count.double() >= float(min_fraction) * largest)
    keep_v = keep_root[label]
    keep_f = keep_v[faces[:, 0]]
    remap = torch.cumsum(keep_v, 0) - 1
    out_faces = remap[faces[keep_f]]
    info = dict(components=int(is_root.sum()), kept=int(keep_root.sum()), largest_faces=largest,
                dropped_faces=m - int(out_faces.shape[0]), dropped_vertices=n - int(keep_v.sum()))
    return verts[keep_v], colours[keep_v], out_faces, info


_VERTEX = [("xyz", "<f4", 3), ("rgb", "u1", 3)]                         # 15 bytes
_FACE = [("n", "u1"), ("idx", "<i4", 3)]                                # 13 bytes
_HEADER = (["property float %s" % a for a in "xyz"] + ["property uchar %s" % a for a in ("red", "green", "blue")],
           ["property list uchar int vertex_indices"])


def save_mesh_ply(verts, colours, faces, path):
    """verts [n, 3] fp32, colours [n, 3] in [0, 1], faces [m, 3] -> binary little-endian .ply: x y z float32 and red green blue uchar
    (rounded as save_points_ply rounds) per vertex, a uchar count of 3 and three int32 indices per face.  -> (n, m)."""
    n, m = int(verts.shape[0]), int(faces.shape[0])
    vr = np.empty(n, dtype=_VERTEX)
    vr["xyz"] = verts.detach().float().cpu().numpy()
    vr["rgb"] = (colours.detach().float().cpu().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).numpy()
    fr = np.empty(m, dtype=_FACE)
    fr["n"] = 3
    fr["idx"] = faces.detach().cpu().numpy().astype("<i4")
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n] + _HEADER[0] + ["element face %d" % m] + _HEADER[1]
    with open(path, "wb") as fh:
        fh.write(("\n".join(lines) + "\nend_header\n").encode("ascii"))
        fh.write(vr.tobytes())
        fh.write(fr.tobytes())
    return n, m


def load_mesh_ply(path):
    """The inverse of ``save_mesh_ply`` -> (verts [n, 3] fp32, colours [n, 3] uint8, faces [m, 3] int64)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    elems = [i for i, ln in enumerate(lines) if ln.startswith("element")]
    if (lines[:2] != ["ply", "format binary_little_endian 1.0"] or len(elems) != 2 or not lines[elems[0]].startswith("element vertex ")
            or not lines[elems[1]].startswith("element face ") or lines[elems[0] + 1:elems[1]] != _HEADER[0]
            or lines[elems[1] + 1:-1] != _HEADER[1]):
        raise ValueError(f"{path}: not a mesh written by save_mesh_ply")
    n, m = int(lines[elems[0]].split()[2]), int(lines[elems[1]].split()[2])
    vr = np.frombuffer(data, dtype=_VERTEX, count=n, offset=end)
    fr = np.frombuffer(data, dtype=_FACE, count=m, offset=end + 15 * n)
    if m and not (fr["n"] == 3).all():
        raise ValueError(f"{path}: faces that are not triangles")
    return torch.from_numpy(vr["xyz"].copy()), torch.from_numpy(vr["rgb"].copy()), torch.from_numpy(fr["idx"].astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------- UV texture
MAX_TEXTURE = 8192


def _atlas_size(n_faces, patch):
    """-> (Wc, T) of the atlas of include/vmv.h ("Texture baking"): cells = ceil(m / 2), Wc = ceil(sqrt(cells)), T = P Wc"""
    m, P = int(n_faces), int(patch)
    if m < 1 or P < 4:
        raise ValueError(f"texture atlas: n_faces must be >= 1 and patch >= 4, got {m} and {P}")
    cells = (m + 1) // 2
    Wc = math.isqrt(cells - 1) + 1
    if P * Wc > MAX_TEXTURE:
        raise ValueError(f"texture atlas: {m} faces at patch {P} need a texture of {P * Wc} px, more than {MAX_TEXTURE}: "
                         f"choose a smaller patch (gs_mesh_texture_patch) or a smaller gs_mesh_res")
    return Wc, P * Wc


def texture_atlas(n_faces, patch=8):
    """The closed-form atlas: two faces share every P x P cell of a T x T texture, cell k at column k % Wc, row k // Wc (rows top-down).
    -> (T, uv [m, 3, 2] fp32): uv[f, corner] = (x, y) in TEXELS (a texel centre is at a half-integer; vt = (x / T, 1 - y / T) in an
    .obj).  Face 2k's corners sit at the cell's origin + (0.5, 0.5), (P - 2.5, 0.5), (0.5, P - 2.5); face 2k + 1's at the cell's far
    corner minus those.  Refuses T > 8192."""
    m, P = int(n_faces), int(patch)
    Wc, T = _atlas_size(m, P)
    f = torch.arange(m)
    k = f // 2
    origin = torch.stack([(k % Wc) * P, (k // Wc) * P], dim=1).to(torch.float32)                       # [m, 2]
    tri = torch.tensor([[0.5, 0.5], [P - 2.5, 0.5], [0.5, P - 2.5]], dtype=torch.float32)              # [3, 2]
    upper = (f % 2 == 1)[:, None, None]
    return T, origin[:, None, :] + torch.where(upper, float(P) - tri[None], tri[None])


def _bake_eager(verts, colours, faces, depth, colour, views, tan_half_fov, patch, T, depth_tol, cos_min, z_min):
    """The contract of vmv_gs_mesh_bake (include/vmv.h) in fp32 torch on verts' device -> (planes [4, T, T], a face index out of range)."""
    dev, P, m, n = verts.device, int(patch), int(faces.shape[0]), int(verts.shape[0])
    V, S = int(depth.shape[0]), int(depth.shape[-1])
    Wc = T // P
    y, x = torch.meshgrid(torch.arange(T, device=dev), torch.arange(T, device=dev), indexing="ij")
    i, j = x % P, y % P
    upper = (i + j) >= P
    f = 2 * ((y // P) * Wc + x // P) + upper
    tri = faces[f.clamp(max=m - 1)]                                     # [T, T, 3]
    in_range = ((tri >= 0) & (tri < n)).all(-1)
    owned = (f < m) & in_range
    bad = (f < m) & ~in_range
    sel = owned.reshape(-1).nonzero()[:, 0]
    tri = tri.reshape(-1, 3)[sel]
    pick = lambda t: t.reshape(-1)[sel].to(torch.float32)
    sb, tb = pick(torch.where(upper, P - 1 - i, i)), pick(torch.where(upper, P - 1 - j, j))
    beta, gamma = (sb / float(P - 3)).clamp(0, 1), (tb / float(P - 3)).clamp(0, 1)
    bg = beta + gamma
    over = bg > 1
    beta, gamma = torch.where(over, beta / bg, beta), torch.where(over, gamma / bg, gamma)
    alpha = 1.0 - beta - gamma
    v0, v1, v2 = (verts[tri[:, c]] for c in range(3))
    p = alpha[:, None] * v0 + beta[:, None] * v1 + gamma[:, None] * v2
    e1, e2 = v1 - v0, v2 - v0                                           # written out (no fused multiply-add): a face that names a vertex twice gives exactly 0
    nrm = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], dim=1)
    length = torch.sqrt((nrm * nrm).sum(1))
    flat = length > 0
    nrm = nrm / torch.where(flat, length, torch.ones_like(length))[:, None]
    acc, W = torch.zeros(sel.shape[0], 3, dtype=torch.float32, device=dev), torch.zeros(sel.shape[0], dtype=torch.float32, device=dev)
    for v in range(V):
        M = views[v]
        pc = p @ M[:3, :3] + M[3, :3]                                   # (xv, yv, z)
        z = pc[:, 2]
        front = flat & (z > z_min)
        inv = 1.0 / (torch.where(front, z, torch.ones_like(z)) * tan_half_fov)
        px, py = ((pc[:, 0] * inv + 1.0) * S - 1.0) * 0.5, ((pc[:, 1] * inv + 1.0) * S - 1.0) * 0.5
        inside = front & (px >= 0) & (px <= S - 1) & (py >= 0) & (py <= S - 1)
        px, py = torch.where(inside, px, torch.zeros_like(px)), torch.where(inside, py, torch.zeros_like(py))
        cos = -((nrm @ M[:3, :3]) * pc).sum(1) / pc.norm(dim=1).clamp_min(1e-30)
        facing = inside & (cos > cos_min)
        d = depth[v].reshape(-1)[torch.floor(py + 0.5).long() * S + torch.floor(px + 0.5).long()]
        hit = facing & (d != 0) & ((d - z).abs() <= depth_tol)
        x0, y0 = torch.floor(px), torch.floor(py)
        tx, ty = (px - x0)[None], (py - y0)[None]
        x0, y0 = x0.long(), y0.long()
        x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
        cm = colour[v].reshape(3, -1)
        c = ((1.0 - ty) * ((1.0 - tx) * cm[:, y0 * S + x0] + tx * cm[:, y0 * S + x1])
             + ty * ((1.0 - tx) * cm[:, y1 * S + x0] + tx * cm[:, y1 * S + x1]))                     # [3, N]
        w = torch.where(hit, cos * cos, torch.zeros_like(cos))
        acc += torch.where(hit[:, None], w[:, None] * c.t(), torch.zeros_like(acc))
        W += w
    c0, c1, c2 = (colours[tri[:, c]] for c in range(3))
    fallback = alpha[:, None] * c0 + beta[:, None] * c1 + gamma[:, None] * c2
    rgb = torch.where((W > 0)[:, None], acc / W.clamp_min(1e-30)[:, None], fallback)
    out = torch.full((4, T * T), 0.5, dtype=torch.float32, device=dev)
    out[3] = -1.0
    out[:3, sel] = rgb.t()
    out[3, sel] = W
    return out.reshape(4, T, T), bad.any()


@torch.no_grad()
def bake_texture(verts, colours, faces, depth, colour, cam_view, tan_half_fov, patch=8, depth_tol=None, cos_min=0.1, z_min=0.05):
    """Blend the views ``colour`` [V, 3, S, S] with depth maps ``depth`` [V, S, S] (view depth, 0 = no surface) seen through ``cam_view``
    [V, 4, 4] (row-vector convention) over the mesh (``verts`` [n, 3], ``colours`` [n, 3], ``faces`` [m, 3] int64) into the atlas of
    ``texture_atlas(m, patch)``: every texel of a face takes, from each view that sees its surface point within ``depth_tol`` of the
    view's depth map at an angle with cos > ``cos_min``, the bilinear colour with weight cos^2; a texel no view sees takes the
    interpolated vertex colours (the contract of vmv_gs_mesh_bake, include/vmv.h).  ``depth_tol`` None: 1 % of the diagonal of the mesh's
    bounding box.  CUDA tensors run the kernel on the current stream; CPU tensors an fp32 torch restatement of the same definition.
    -> (texture [4, T, T] fp32 on verts' device: R, G, B and the weight W (0: fell back, -1: no face), uv [m, 3, 2] in texels, info =
    dict(size, texels (those of a face), baked (the share of them with W > 0), fallback (the share with W == 0)))."""
    n, m, P = int(verts.shape[0]), int(faces.shape[0]), int(patch)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    T, uv = texture_atlas(m, P)
    if n < 1:
        raise ValueError("bake_texture: a mesh without vertices")
    if not 0.0 <= float(cos_min) < 1.0:
        raise ValueError(f"bake_texture: cos_min must be in [0, 1), got {cos_min}")
    dev = verts.device
    verts, colours = verts.to(torch.float32).contiguous(), colours.to(dev, torch.float32).contiguous()
    if depth_tol is None:
        depth_tol = 0.01 * float((verts.max(0).values - verts.min(0).values).norm())
    if not float(depth_tol) > 0:
        raise ValueError(f"bake_texture: depth_tol must be positive, got {depth_tol}")
    d, col, views = _view_tensors(depth, colour, cam_view, dev)
    V, S = d.shape[:2]
    if dev.type != "cuda":
        tex, bad = _bake_eager(verts, colours, faces, d, col, views.reshape(V, 4, 4), float(tan_half_fov), P, T, float(depth_tol), float(cos_min), float(z_min))
        _raise_status(L.MESH_STATUS_RANGE if bool(bad) else 0, "bake_texture", n)
    else:
        from .ops import _stream_ptr
        faces = _kernel_faces(faces)
        tex = torch.empty(4, T, T, dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        p = L.GsMeshBakeParams()
        p.verts, p.vert_colours, p.faces = verts.data_ptr(), colours.data_ptr(), faces.data_ptr()
        p.face_stride, p.n_faces, p.n_vertices = int(faces.stride(0)), m, n
        p.depth, p.colour, p.views, p.n_views, p.size, p.tan_half_fov = d.data_ptr(), col.data_ptr(), views.data_ptr(), V, S, float(tan_half_fov)
        p.z_min, p.depth_tol, p.cos_min, p.patch, p.tex_size = float(z_min), float(depth_tol), float(cos_min), P, T
        p.out, p.plane_stride, p.status = tex.data_ptr(), T * T, status.data_ptr()
        L.check(L.load().vmv_gs_mesh_bake(C.byref(p), _stream_ptr()), "gs_mesh_bake")
        _raise_status(int(status), "bake_texture", n)
    owned = int((tex[3] >= 0).sum())
    baked = int((tex[3] > 0).sum())
    info = dict(size=T, texels=owned, baked=baked / max(owned, 1), fallback=(owned - baked) / max(owned, 1))
    return tex, uv, info


_MATERIAL = "baked"


def save_mesh_obj(verts, faces, uv, texture, path):
    """-> ``path``.obj (v, vt = (x / T, 1 - y / T) per face corner, f a/ta b/tb c/tc, mtllib, usemtl), ``path``.mtl (one material whose
    map_Kd is the texture) and ``path``_tex.png (the R, G, B planes of ``texture`` [>= 3, T, T] as 8-bit RGB, rounded as save_mesh_ply
    rounds).  Vertices are not duplicated: an .obj has per-corner UVs.  -> (n, m, T)."""
    from PIL import Image
    n, m, T = int(verts.shape[0]), int(faces.shape[0]), int(texture.shape[-1])
    base = os.path.basename(path)
    rgb = (texture[:3].detach().float().cpu().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    Image.fromarray(rgb, "RGB").save(path + "_tex.png")
    with open(path + ".mtl", "w") as fh:
        fh.write(f"newmtl {_MATERIAL}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {base}_tex.png\n")
    v = verts.detach().float().cpu().numpy()
    t = uv.detach().double().cpu().reshape(-1, 2).numpy()
    f = faces.detach().cpu().numpy() + 1
    lines = [f"mtllib {base}.mtl", f"usemtl {_MATERIAL}"]
    lines += ["v %.9g %.9g %.9g" % (a, b, c) for a, b, c in v.tolist()]
    lines += ["vt %.8f %.8f" % (x / T, 1.0 - y / T) for x, y in t.tolist()]
    lines += ["f %d/%d %d/%d %d/%d" % (a, 3 * k + 1, b, 3 * k + 2, c, 3 * k + 3) for k, (a, b, c) in enumerate(f.tolist())]
    with open(path + ".obj", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return n, m, T


def load_mesh_obj(path):
    """The inverse of ``save_mesh_obj`` -> (verts [n, 3] fp32, faces [m, 3] int64, uv [m, 3, 2] fp32 in texels, texture [T, T, 3] uint8)."""
    from PIL import Image
    v, vt, fv, ft, mtl = [], [], [], [], None
    with open(path + ".obj") as fh:
        for ln in fh:
            w = ln.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                vt.append([float(x) for x in w[1:3]])
            elif w[0] == "f":
                if len(w) != 4:
                    raise ValueError(f"{path}.obj: faces that are not triangles")
                pairs = [x.split("/") for x in w[1:]]
                fv.append([int(a[0]) - 1 for a in pairs])
                ft.append([int(a[1]) - 1 for a in pairs])
            elif w[0] == "mtllib":
                mtl = w[1]
    if mtl is None:
        raise ValueError(f"{path}.obj: not a mesh written by save_mesh_obj")
    image = None
    with open(os.path.join(os.path.dirname(path), mtl)) as fh:
        for ln in fh:
            w = ln.split()
            if w and w[0] == "map_Kd":
                image = os.path.join(os.path.dirname(path), w[1])
    if image is None:
        raise ValueError(f"{path}.mtl: no map_Kd")
    tex = torch.from_numpy(np.array(Image.open(image).convert("RGB")))
    T = int(tex.shape[0])
    verts = torch.tensor(v, dtype=torch.float64).to(torch.float32).reshape(-1, 3)
    faces = torch.tensor(fv, dtype=torch.int64).reshape(-1, 3)
    t = torch.tensor(vt, dtype=torch.float64).reshape(-1, 2)[torch.tensor(ft, dtype=torch.int64).reshape(-1, 3)]
    uv = torch.stack([t[..., 0] * T, (1.0 - t[..., 1]) * T], dim=-1).to(torch.float32)
    return verts, faces, uv, tex
