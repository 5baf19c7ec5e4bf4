"""The yardstick of the component labelling (csrc/gs_mesh_cc.hip, gs_mesh.mesh_components / drop_small_components): a plain sequential
union-find with path compression and smallest-index roots, the floater filter restated on top of it, and the graphs the CPU and the GPU
tests label.  Python and numpy only: no scipy, nothing of the code under test (the analytic floater fixture goes through
``surface_nets``, which this work does not touch).  Every case is computed once, shared, never modified."""
import functools

import numpy as np
import torch


def components_ref(faces, n):
    """faces [m, 3] integers, n vertices -> (label [n] int64: the smallest vertex index of each vertex's component, face_count [n] int64:
    faces per component at its label, 0 elsewhere).  A face with an index outside [0, n) is skipped whole."""
    parent = list(range(n))

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < n)).all(axis=1)]
    for a, b, c in f.tolist():
        for x, y in ((a, b), (a, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)                      # the smaller index stays the root
    label = np.array([find(v) for v in range(n)], dtype=np.int64).reshape(n)
    count = np.zeros(n, dtype=np.int64)
    if len(f):
        np.add.at(count, label[f[:, 0]], 1)
    return label, count


def drop_ref(verts, colours, faces, min_fraction=0.0, min_faces=0):
    """the floater filter on numpy arrays: a component stays iff its faces >= min_faces and >= min_fraction x the largest count; order kept,
    indices remapped -> (verts, colours, faces, info)"""
    verts, colours, faces = np.asarray(verts), np.asarray(colours), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = len(verts)
    label, count = components_ref(faces, n)
    roots = [r for r in range(n) if label[r] == r]
    largest = int(count.max()) if n else 0
    kept = [r for r in roots if count[r] >= min_faces and count[r] >= min_fraction * largest]
    keep_v = np.isin(label, kept) if n else np.zeros(0, dtype=bool)
    keep_f = keep_v[faces[:, 0]] if len(faces) else np.zeros(0, dtype=bool)
    remap = np.cumsum(keep_v) - 1
    out = remap[faces[keep_f]].reshape(-1, 3)
    info = dict(components=len(roots), kept=len(kept), largest_faces=largest, dropped_faces=len(faces) - len(out),
                dropped_vertices=n - int(keep_v.sum()))
    return verts[keep_v], colours[keep_v], out, info


# --------------------------------------------------------------------------------------------------------------------- the graphs
def _strip(T, first=0):
    i = np.arange(T, dtype=np.int64) + first
    return np.stack([i, i + 1, i + 2], axis=1)


def _renumber(faces, n, order):
    if order == "forward":
        return faces
    new = np.arange(n - 1, -1, -1, dtype=np.int64) if order == "reverse" else np.random.default_rng(11).permutation(n).astype(np.int64)
    return new[faces]


def _build(name):
    """-> (faces [m, 3] int64, n)"""
    rng = np.random.default_rng(5)
    if name == "empty":
        return np.zeros((0, 3), dtype=np.int64), 7
    if name == "one-face":
        return np.array([[4, 1, 2]], dtype=np.int64), 6
    if name.startswith("random-"):                                     # 255 / 256 / 257 faces over 300 vertices: the partial last block
        return rng.integers(0, 300, size=(int(name.split("-")[1]), 3), dtype=np.int64), 300
    if name.startswith("strip-"):                                      # 65 536 triangles over 65 538 vertices: long chains
        return _renumber(_strip(65536), 65538, name.split("-")[1]), 65538
    if name == "hub":                                                  # every union re-hooks the largest index: one contended address
        i = np.arange(65536, dtype=np.int64)
        return np.stack([np.full_like(i, 2 * 65536), 2 * i, 2 * i + 1], axis=1), 2 * 65536 + 1
    if name == "tetrahedra":                                           # vertex j of tetrahedron t is t + 4096 j
        t = np.arange(4096, dtype=np.int64)[:, None, None]
        return (t + 4096 * np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)[None]).reshape(-1, 3), 4 * 4096
    if name == "bridge":                                               # two strips and the one face that joins them, listed last
        a, b = _strip(700), _strip(500, first=1000)
        return np.concatenate([a, b, np.array([[1300, 350, 351]], dtype=np.int64)]), 1502
    if name == "degenerate":                                           # (a, a, b), (a, a, a), duplicates, isolated vertices 0, 5, 11, 19
        return np.array([[3, 3, 7], [7, 9, 9], [2, 2, 2], [1, 4, 6], [1, 4, 6], [6, 4, 1], [10, 8, 10], [12, 13, 14], [14, 15, 16],
                         [18, 17, 18], [17, 17, 16]], dtype=np.int64), 20
    if name == "floaters":
        return floater_mesh()[2].numpy(), int(floater_mesh()[0].shape[0])
    raise KeyError(name)


CPU_CASES = ["empty", "one-face", "random-255", "random-256", "random-257", "strip-forward", "strip-reverse", "strip-permuted", "hub",
             "tetrahedra", "bridge", "degenerate", "floaters"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (faces [m, 3] int64 tensor, n, label [n] int64 tensor, face_count [n] int64 tensor) of the reference"""
    faces, n = _build(name)
    label, count = components_ref(faces, n)
    return torch.from_numpy(np.ascontiguousarray(faces)), n, torch.from_numpy(label), torch.from_numpy(count)


# ------------------------------------------------------------------------------------------------------- the analytic floater mesh
BALLS = [((0.05, -0.03, 0.02), 0.45)] + [((0.62 * np.cos(a), 0.62 * np.sin(a), h), r) for a, h, r in
                                         ((0.3, 0.5, 0.09), (1.7, -0.55, 0.07), (2.9, 0.1, 0.11), (4.0, 0.6, 0.06), (5.2, -0.4, 0.08))]
FLOATER_FACES = (3052, 188, 124, 92, 72, 48)                           # per component; 1 800 vertices, 3 576 faces


@functools.lru_cache(maxsize=None)
def floater_mesh():
    """six balls on the R = 32 grid of half-width 0.8: the field is the min over their signed distances, divided by 3 voxels and
    clamped (test_gs_mesh_cpu._analytic) -> surface_nets' (verts, colours, faces)"""
    from tests.test_gs_mesh_cpu import _analytic, _grid
    from videomv_amd.gs_mesh import surface_nets
    x, y, z, voxel, o = _grid(32, 0.8)
    sd = torch.stack([((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2).sqrt() - r for c, r in BALLS]).min(0).values
    f, valid = _analytic(sd, voxel)
    return surface_nets(f, valid, o, voxel, colour=torch.stack([x, y, z]).float() * 0.5 + 0.5)
