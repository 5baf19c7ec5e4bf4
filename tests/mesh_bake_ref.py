"""The yardstick of the texture-baking kernel (csrc/gs_mesh_bake.hip): the definition of include/vmv.h ("Texture baking"), restated from the
header text in vectorised torch, fp64 by default.  ``dtype=torch.float32`` evaluates the SAME definition in fp32 on the CPU: its error
against fp64 is what the number format costs, and ten times that is the bound the tests hold the kernel and the host's fallback to.
Next to the planes it returns, per texel, how far the nearest of its decisions was from its threshold, and the analytic coloured-sphere
scene of the quality test.  Plain Python: no fixtures."""
import functools
import math

import torch

from tests.gs_tsdf_ref import CLEAR, HALF, SPHERE, TAN, f32, integrate_ref, sphere_depth  # noqa: F401  (CLEAR, TAN: re-exported)


def atlas_ref(n_faces, patch):
    """-> (T, Wc, face [T, T] int64 (the face that owns the texel; >= n_faces: none), s, t [T, T] (the texel centre in its face's frame))"""
    m, P = int(n_faces), int(patch)
    cells = (m + 1) // 2
    Wc = math.isqrt(cells)
    Wc += Wc * Wc < cells
    T = P * Wc
    y, x = torch.meshgrid(torch.arange(T), torch.arange(T), indexing="ij")
    i, j = x % P, y % P
    k = (y // P) * Wc + (x // P)
    lower = i + j <= P - 1
    face = torch.where(lower, 2 * k, 2 * k + 1)
    s = torch.where(lower, i + 0.5, P - i - 0.5)
    t = torch.where(lower, j + 0.5, P - j - 0.5)
    return T, Wc, face, s.double(), t.double()


def bake_ref(verts, colours, faces, depth, colour, views, tan_half_fov, patch, depth_tol, cos_min=0.1, z_min=0.05, dtype=torch.float64):
    """verts [n, 3], colours [n, 3], faces [m, 3] int64, depth [V, S, S], colour [V, 3, S, S], views [V, 4, 4] (row-vector convention)
    -> dict(planes [4, T, T] (R, G, B, W), margin [T, T] fp64, bad (a face index was out of range), point [T, T, 3] (the texel's surface
    point), vertex_rgb [T, T, 3] (alpha c0 + beta c1 + gamma c2), T).
    ``margin`` is the smallest distance of any of the texel's decisions to its threshold, each counted where the walk reaches it:
    |z - z_min| / z_min; |px|, |px - (size - 1)| (likewise py); the distance of px + 0.5 (py + 0.5) to the nearest integer; |cos - cos_min|;
    ||d - z| - depth_tol| / depth_tol where d != 0.  A texel whose margin is at least CLEAR takes the same branches in fp32."""
    P, m, n = int(patch), int(faces.shape[0]), int(verts.shape[0])
    V, S = int(depth.shape[0]), int(depth.shape[-1])
    T, Wc, face, s, t = atlas_ref(m, P)
    verts, colours = verts.to(dtype), colours.to(dtype)
    depth, colour, views = depth.to(dtype).reshape(V, S, S), colour.to(dtype).reshape(V, 3, S, S), views.to(dtype).reshape(V, 4, 4)
    has_face = face < m
    idx = faces[face.clamp(max=m - 1)]                                  # [T, T, 3]
    in_range = ((idx >= 0) & (idx < n)).all(-1)
    bad = bool((has_face & ~in_range).any())
    owned = has_face & in_range
    idx = idx.clamp(0, n - 1)
    beta = ((s.to(dtype) - 0.5) / (P - 3)).clamp(0, 1)
    gamma = ((t.to(dtype) - 0.5) / (P - 3)).clamp(0, 1)
    both = beta + gamma
    beta, gamma = torch.where(both > 1, beta / both, beta), torch.where(both > 1, gamma / both, gamma)
    alpha = 1 - beta - gamma
    v0, v1, v2 = verts[idx[..., 0]], verts[idx[..., 1]], verts[idx[..., 2]]
    point = alpha[..., None] * v0 + beta[..., None] * v1 + gamma[..., None] * v2
    e1, e2 = v1 - v0, v2 - v0                                           # written out: products and differences rounded one by one, so that
    cross = torch.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],                          # a face that names a vertex twice
                         e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],                          # gives exactly zero in every format
                         e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], dim=-1)
    length = torch.sqrt((cross * cross).sum(-1))
    alive = owned & (length > 0)
    normal = cross / torch.where(length > 0, length, torch.ones_like(length))[..., None]
    total, W = torch.zeros(T, T, 3, dtype=dtype), torch.zeros(T, T, dtype=dtype)
    margin = torch.full((T, T), float("inf"), dtype=torch.float64)

    def near(reached, distance):
        nonlocal margin
        margin = torch.where(reached, torch.minimum(margin, distance.abs().double()), margin)
    for v in range(V):
        M = views[v]
        xv = point[..., 0] * M[0, 0] + point[..., 1] * M[1, 0] + point[..., 2] * M[2, 0] + M[3, 0]
        yv = point[..., 0] * M[0, 1] + point[..., 1] * M[1, 1] + point[..., 2] * M[2, 1] + M[3, 1]
        z = point[..., 0] * M[0, 2] + point[..., 1] * M[1, 2] + point[..., 2] * M[2, 2] + M[3, 2]
        near(alive, (z - z_min) / z_min)
        front = alive & (z > z_min)
        zs = torch.where(front, z, torch.ones_like(z))
        px = ((xv / (zs * tan_half_fov) + 1) * S - 1) / 2
        py = ((yv / (zs * tan_half_fov) + 1) * S - 1) / 2
        for q in (px, py):
            near(front, q)
            near(front, q - (S - 1))
        inside = front & (px >= 0) & (px <= S - 1) & (py >= 0) & (py <= S - 1)
        for q in (px, py):
            near(inside, (q + 0.5) - torch.round(q + 0.5))
        px, py = torch.where(inside, px, torch.zeros_like(px)), torch.where(inside, py, torch.zeros_like(py))
        nc = [normal[..., 0] * M[0, c] + normal[..., 1] * M[1, c] + normal[..., 2] * M[2, c] for c in range(3)]
        cos = -(nc[0] * xv + nc[1] * yv + nc[2] * z) / torch.sqrt(xv * xv + yv * yv + z * z).clamp_min(1e-300 if dtype == torch.float64 else 1e-30)
        near(inside, cos - cos_min)
        facing = inside & (cos > cos_min)
        d = depth[v][torch.floor(py + 0.5).long(), torch.floor(px + 0.5).long()]
        surface = facing & (d != 0)
        near(surface, ((d - z).abs() - depth_tol) / depth_tol)
        hit = surface & ~((d - z).abs() > depth_tol)
        x0, y0 = torch.floor(px).long(), torch.floor(py).long()
        x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
        tx, ty = (px - x0)[..., None], (py - y0)[..., None]
        img = colour[v].permute(1, 2, 0)                                # [S, S, 3]
        c = (1 - ty) * ((1 - tx) * img[y0, x0] + tx * img[y0, x1]) + ty * ((1 - tx) * img[y1, x0] + tx * img[y1, x1])
        w = torch.where(hit, cos * cos, torch.zeros_like(cos))
        total = total + torch.where(hit[..., None], w[..., None] * c, torch.zeros_like(c))
        W = W + w
    c0, c1, c2 = colours[idx[..., 0]], colours[idx[..., 1]], colours[idx[..., 2]]
    vertex_rgb = alpha[..., None] * c0 + beta[..., None] * c1 + gamma[..., None] * c2
    rgb = torch.where((W > 0)[..., None], total / torch.where(W > 0, W, torch.ones_like(W))[..., None], vertex_rgb)
    rgb = torch.where(owned[..., None], rgb, torch.full_like(rgb, 0.5))
    W = torch.where(owned, W, -torch.ones_like(W))
    return dict(planes=torch.cat([rgb.permute(2, 0, 1), W[None]]), margin=margin, bad=bad, point=point, vertex_rgb=vertex_rgb, T=T)


# --------------------------------------------------------------------------------------------- the analytic coloured sphere
# the colour of the sphere's surface as a function of the direction from its centre: per channel 0.5 + 0.5 sin(12 a . dir + phase).  On
# SPHERE (r = 0.32) one period is 0.17 of arc: 2.5 voxels of the 16^3 volume over HALF and 5 of the 32^3 one — detail a colour per voxel
# cannot carry — and 7 pixels of a 48-px view from distance 1.6, 18 of a 128-px one, which a bilinear fetch follows.
_AXES = torch.tensor([[0.6, 0.0, 0.8], [0.0, 0.8, -0.6], [0.8, 0.6, 0.0]], dtype=torch.float64)
_PHASE = torch.tensor([0.3, 1.7, 4.1], dtype=torch.float64)
OMEGA = 12.0


def direction_colour(direction):
    """[..., 3] unit directions -> [..., 3] colours in [0, 1], fp64"""
    return 0.5 + 0.5 * torch.sin(OMEGA * (direction.double() @ _AXES.t()) + _PHASE)


def surface_colour(points, centre):
    """the true colour of the sphere's surface under every point (seen from the centre) -> [..., 3] fp64"""
    d = points.double() - torch.tensor(list(centre), dtype=torch.float64)
    return direction_colour(d / d.norm(dim=-1, keepdim=True).clamp_min(1e-300))


def sphere_render(cam_views, S, centre, r, tan_half_fov=TAN):
    """The coloured sphere seen per pixel CENTRE of every view: depth [V, S, S] (gs_tsdf_ref.sphere_depth, 0 where the ray misses) and
    colour [V, 3, S, S] (the surface colour at the point the ray hits, 0.5 where it misses), fp64"""
    ndc = (2.0 * torch.arange(S, dtype=torch.float64) + 1.0) / S - 1.0
    dy, dx = torch.meshgrid(ndc * tan_half_fov, ndc * tan_half_fov, indexing="ij")
    depths, colours = [], []
    for cv in cam_views:
        cv = cv.double()
        z = sphere_depth(cv, S, centre, r, tan_half_fov)
        cam = torch.stack([dx * z, dy * z, z], dim=-1)                  # [S, S, 3] in view space
        world = (cam - cv[3, :3]) @ torch.inverse(cv[:3, :3])
        col = torch.where((z > 0)[..., None], surface_colour(world, centre), torch.full_like(world, 0.5))
        depths.append(z)
        colours.append(col.permute(2, 0, 1))
    return torch.stack(depths), torch.stack(colours)


# ---------------------------------------------------------------------------------------------------------------- shared cases
def depth_tol_of(R, half=HALF):
    """two voxels of the R^3 volume over the cube of half-width ``half``, as a C float: the entrance's default"""
    return f32(2.0 * (2.0 * half / R))


@functools.lru_cache(maxsize=None)
def sphere_bake_case(V, S, R, P, variant="plain"):
    """SPHERE rendered analytically from ``_cams(V)`` at S px, fused at R^3 by the fp64 TSDF reference, extracted by surface_nets, baked
    at patch P by both evaluations of the definition.  ``variant``: "odd" drops the last face, "one" keeps the first face alone,
    "degenerate" makes face 5 name one vertex twice.  Computed once, shared, never modified."""
    from tests.test_gs_gpu import _cams
    from videomv_amd.gs_mesh import TsdfVolume
    centre, r = SPHERE[0]
    cv, _ = _cams(V)
    depth, colour = sphere_render(cv, S, centre, r)
    depth, colour = depth.float(), colour.float()
    vol = TsdfVolume(R, HALF, device="cpu")
    integrate_ref(vol, depth, cv, TAN, colour=colour)
    verts, cols, faces = vol.extract()
    if variant == "odd":
        faces = faces[:-1] if faces.shape[0] % 2 == 0 else faces[:-2]
    elif variant == "one":
        # m = 1: one triangle that touches the sphere where view 0 sees it head-on and leaves it towards its corners, 0.5 from the touching
        # point, where it floats 0.3 above the surface (more than ``tol``) or beside the silhouette: its middle bakes, its corners fall back
        u = torch.inverse(cv[0].double())[3, :3] - torch.tensor(list(centre), dtype=torch.float64)
        u = u / u.norm()
        e1 = torch.linalg.cross(u, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
        e1 = e1 / e1.norm()
        e2 = torch.linalg.cross(u, e1)                                  # e1 x e2 = u: counter-clockwise corners face the camera
        touch = torch.tensor(list(centre), dtype=torch.float64) + r * u
        verts = torch.stack([touch + 0.5 * (math.cos(a) * e1 + math.sin(a) * e2) for a in (0.3, 0.3 + 2 * math.pi / 3, 0.3 + 4 * math.pi / 3)]).float()
        cols, faces = torch.tensor([[0.9, 0.1, 0.2], [0.2, 0.8, 0.1], [0.1, 0.3, 0.7]]), torch.tensor([[0, 1, 2]])
    elif variant == "degenerate":
        faces = faces.clone()
        faces[5, 2] = faces[5, 1]
    else:
        assert variant == "plain"
    return _case(dict(V=V, S=S, R=R, P=P, variant=variant, views=cv, depth=depth, colour=colour, verts=verts, cols=cols,
                      faces=faces.contiguous(), tol=depth_tol_of(R), centre=centre, r=r))


def _case(case, **kw):
    """adds both evaluations of the definition (fp64: ``ref``; fp32: ``ref32``) to a case (``tan``: the C float of tan(fovy / 2), TAN's by default)"""
    args = (case["verts"], case["cols"], case["faces"], case["depth"], case["colour"], case["views"], case.get("tan", f32(TAN)), case["P"], case["tol"])
    case["ref"] = bake_ref(*args, cos_min=f32(0.1), z_min=f32(0.05), **kw)
    case["ref32"] = bake_ref(*args, cos_min=f32(0.1), z_min=f32(0.05), dtype=torch.float32, **kw)
    return case


def compare(name, planes, case, need_both=True, max_unclear=0.01):
    """On the clear texels: the sets {W > 0}, {W == 0}, {W == -1} exact, RGB and W within 10 x the fp32 evaluation's own error against
    fp64; the unclear share <= 1 % (``max_unclear`` None: not asked of a mesh the test did not choose).  Prints every figure before it
    asserts -> the figures."""
    ref, ref32, got = case["ref"]["planes"], case["ref32"]["planes"].double(), planes.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    clear = case["ref"]["margin"] >= CLEAR
    unclear = 1.0 - float(clear.double().mean())
    sets = {k: int((sel(got[3]) != sel(ref[3]))[clear].sum()) for k, sel in (("baked", lambda w: w > 0), ("fallback", lambda w: w == 0), ("none", lambda w: w == -1))}
    same = clear & ((got[3] > 0) == (ref[3] > 0)) & ((ref32[3] > 0) == (ref[3] > 0))
    fig = {}
    for what, sl in (("rgb", slice(0, 3)), ("w", slice(3, 4))):
        fig[what] = (float((got[sl] - ref[sl])[:, same].abs().max()), 10.0 * float((ref32[sl] - ref[sl])[:, same].abs().max()))
    counts = dict(baked=int((ref[3] > 0).sum()), fallback=int((ref[3] == 0).sum()), none=int((ref[3] == -1).sum()))
    print(f"{name}: T {case['ref']['T']}, {case['faces'].shape[0]} faces, unclear {100 * unclear:.2f} %, RGB error {fig['rgb'][0]:.2e} "
          f"(bound {fig['rgb'][1]:.2e}), W error {fig['w'][0]:.2e} (bound {fig['w'][1]:.2e}), texels in the wrong set {sets}, reference {counts}")
    assert max_unclear is None or unclear <= max_unclear
    assert sets == dict(baked=0, fallback=0, none=0)
    assert fig["rgb"][0] <= fig["rgb"][1] and fig["w"][0] <= fig["w"][1], fig
    if need_both:
        assert counts["baked"] > 0 and counts["fallback"] > 0, counts      # the case reaches the baked and the fallback branch
    return fig
