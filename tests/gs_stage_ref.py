"""TEST INFRASTRUCTURE (CPU): the Gaussian rasteriser's forward pass restated STAGE BY STAGE, with one comparator per stage.

Written from the definitions of include/vmv.h and the header of oracle/gs_ref.py, not from the kernels.  Every function takes and returns
plain CPU tensors, so tests/test_gs_stages_cpu.py drives them with arrays simulated from the fp32 oracle and
tests/test_gs_stages_gpu.py with the arrays the kernels left on the device (``GaussianRenderer.binning`` / ``binning_view``).

  preprocess   ``preprocess_ref``: oracle.gs_ref.preprocess on fp64 inputs, plus what it does not return — the radius before the ceil,
               the rectangle edges before the floor, det — and the records "on a boundary", where an fp32 evaluation may legitimately
               take the neighbouring integer decision.  ``check_preprocess`` holds tiles_touched / rect to it: exact away from the
               boundary records, one of the neighbouring decisions on them.  ``preprocess_errors`` measures xy / conic / depth.
  binning      ``binning_ref``: integers only.  From the kernel's OWN tiles_touched, rect and depth bits, the Gaussian indices of every
               (view, tile) in (depth bits, index) order.  ``check_binning`` holds ranges, sorted values and sorted keys to it: equality,
               no tolerance, no exclusion; per-view (64-bit tile << 32 | depth keys) and batched (32-bit (view, tile) keys) form.
  blend        ``blend_ref``: per pixel in fp64 (or fp32, to measure what fp32 arithmetic alone costs) over the per-tile lists and the
               kernel's own fp32 xy / conic / opacity / depth: clamped image, alpha, final T, n_contrib, expected and median depth, and
               the pixels that sit on a decision (``ambiguous``).  ``check_blend`` holds every other pixel to a per-pixel bound.
"""
import math

import torch

from oracle.gs_ref import TILE, preprocess, quat_to_rot
from tests.gs_depth_ref import AMBIGUOUS_CAP, AMBIGUOUS_MARGIN, staging_scene
from tests.test_gs_fit_gpu import _cams, _scene

FOVY = 39.6
TAN = math.tan(0.5 * math.radians(FOVY))
BG = (0.3, 0.5, 0.7)
Z_NEAR, Z_MARGIN, PX_MARGIN, DET_MARGIN = 0.2, 1e-6, 1e-3, 1e-12      # the boundary-record margins
DECISION_MARGIN = 1e-4                                              # the ambiguous-pixel margin (relative)
PIXEL_FLOOR, FP32_FACTOR = 2e-5, 8.0                                # per-pixel bound = max(floor, factor x the fp32 CPU evaluation's error)
BOUNDARY_CAP = 0.01


# ---------------------------------------------------------------------------------------------------------------- preprocess
@torch.no_grad()
def preprocess_ref(gaussians, view, view_proj, size, tan_half_fov=TAN):
    """gaussians [N, 14], one view, all taken to fp64 -> the oracle's dict (valid, depth, xy, conic, radius, rect) plus
    touched [N] (tiles of the rectangle, 0 where culled), radius_raw [N] = 3 sqrt(lambda) before the ceil, edges [N, 4] = the
    rectangle edges in pixels before the / 16 and the floor (x - r, y - r, x + r + 15, y + r + 15), det [N], and boundary [N]:
    |z - 0.2| < 1e-6, or, for a record in front of the near plane, radius_raw within 1e-3 of an integer, an edge within 1e-3 px of a
    multiple of 16, or |det| < 1e-12."""
    g, V, M = gaussians.double(), view.double(), view_proj.double()
    pp = preprocess(g[:, 0:3], g[:, 4:7], g[:, 7:11], V, M, size, tan_half_fov)
    # the terms the oracle keeps to itself, by its formulas (header of oracle/gs_ref.py)
    pv = torch.cat([g[:, 0:3], torch.ones(g.shape[0], 1, dtype=torch.float64)], dim=1) @ V
    tz = pv[:, 2]
    focal, lim = size / (2.0 * tan_half_fov), 1.3 * tan_half_fov
    tx, ty = torch.clamp(pv[:, 0] / tz, -lim, lim) * tz, torch.clamp(pv[:, 1] / tz, -lim, lim) * tz
    J = torch.zeros(g.shape[0], 2, 3, dtype=torch.float64)
    J[:, 0, 0] = J[:, 1, 1] = focal / tz
    J[:, 0, 2], J[:, 1, 2] = -focal * tx / (tz * tz), -focal * ty / (tz * tz)
    R = quat_to_rot(g[:, 7:11])
    T = J @ V[:3, :3].transpose(0, 1)
    cov = T @ (R @ torch.diag_embed(g[:, 4:7] ** 2) @ R.transpose(1, 2)) @ T.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    mid = 0.5 * (a + c)
    radius_raw = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1)))
    front = tz > Z_NEAR
    assert torch.equal(torch.ceil(radius_raw)[front], pp["radius"][front]), "the restated covariance is not the oracle's"
    r, x, y = pp["radius"], pp["xy"][:, 0], pp["xy"][:, 1]
    edges = torch.stack([x - r, y - r, x + r + (TILE - 1), y + r + (TILE - 1)], dim=1)
    near_int = lambda v, step: (v - step * torch.round(v / step)).abs() < PX_MARGIN
    boundary = (tz - Z_NEAR).abs() < Z_MARGIN
    boundary |= (tz > Z_NEAR - Z_MARGIN) & (near_int(radius_raw, 1.0) | near_int(edges, float(TILE)).any(dim=1) | (det.abs() < DET_MARGIN))
    rect = pp["rect"]
    touched = torch.where(pp["valid"], (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]), torch.zeros_like(rect[:, 0]))
    return dict(pp, touched=touched, radius_raw=radius_raw, edges=edges, det=det, boundary=boundary)


def _neighbour_decisions(ref, i, size):
    """For boundary record ``i``: the rectangles an fp32 evaluation may arrive at — for either neighbouring radius, every edge floored
    from either side of its margin — and whether culling it is one of the decisions."""
    grid = (size + TILE - 1) // TILE
    clampi = lambda v: max(0, min(grid, int(math.floor(v))))
    raw, (x, y) = float(ref["radius_raw"][i]), (float(v) for v in ref["xy"][i])
    cull = abs(float(ref["depth"][i]) - Z_NEAR) < Z_MARGIN or abs(float(ref["det"][i])) < DET_MARGIN
    rects = []
    for r in {math.ceil(raw - PX_MARGIN), math.ceil(raw + PX_MARGIN)}:
        sets = [{clampi((e - PX_MARGIN) / TILE), clampi((e + PX_MARGIN) / TILE)} for e in (x - r, y - r, x + r + TILE - 1, y + r + TILE - 1)]
        rects.append(sets)
        cull |= any((x1 - x0) * (y1 - y0) <= 0 for x0 in sets[0] for y0 in sets[1] for x1 in sets[2] for y1 in sets[3])
    return rects, cull


def check_preprocess(ref, touched, rect, size, label=""):
    """One view of the kernel's tiles_touched [N] and rect [N, 4] against ``preprocess_ref``.  Away from boundary records culled / valid,
    tiles_touched and rect are EXACT.  On a boundary record the kernel's answer is one of the neighbouring decisions: culled where that
    is one, else a rectangle whose four edges belong to ONE of the two neighbouring radii.  Every valid record's tiles_touched is its
    rectangle's area.  -> the boundary share."""
    touched, rect = touched.long().cpu(), rect.long().cpu()
    kvalid, clear = touched > 0, ~ref["boundary"]
    bad = clear & (kvalid != ref["valid"])
    assert not bool(bad.any()), f"{label}: culled / valid differs at records {torch.nonzero(bad).flatten().tolist()[:8]}"
    bad = clear & (touched != ref["touched"])
    assert not bool(bad.any()), f"{label}: tiles_touched differs at records {torch.nonzero(bad).flatten().tolist()[:8]}"
    bad = clear & ref["valid"] & (rect != ref["rect"]).any(dim=1)
    assert not bool(bad.any()), f"{label}: rect differs at records {torch.nonzero(bad).flatten().tolist()[:8]}"
    area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    assert torch.equal(area[kvalid], touched[kvalid]), f"{label}: tiles_touched is not the rectangle's area"
    for i in torch.nonzero(ref["boundary"]).flatten().tolist():
        if float(ref["depth"][i]) <= Z_NEAR - Z_MARGIN:
            assert not bool(kvalid[i]), f"{label}: record {i} is behind the near plane"
            continue
        rects, cull = _neighbour_decisions(ref, i, size)
        if not bool(kvalid[i]):
            assert cull, f"{label}: boundary record {i} culled, which is no neighbouring decision"
        else:
            k = [int(v) for v in rect[i]]
            assert any(all(k[j] in sets[j] for j in range(4)) for sets in rects), f"{label}: boundary record {i} rect {k} fits neither radius"
    return float(ref["boundary"].double().mean())


def preprocess_errors(ref, depth, xy, conic, mask):
    """Largest difference of an fp32 preprocess (the oracle's or the kernel's) from ``preprocess_ref`` over the records of ``mask``:
    xy in pixels, conic relative to the record's largest conic entry, depth relative."""
    if not bool(mask.any()):
        return dict(xy=0.0, conic=0.0, depth=0.0)
    m = mask
    dc = (conic.double()[m] - ref["conic"][m]).abs().max(dim=1).values / ref["conic"][m].abs().max(dim=1).values
    return dict(xy=float((xy.double()[m] - ref["xy"][m]).abs().max()), conic=float(dc.max()),
                depth=float(((depth.double()[m] - ref["depth"][m]).abs() / ref["depth"][m]).max()))


# ---------------------------------------------------------------------------------------------------------------- binning
def depth_bits(depth):
    """fp32 depths -> their bit patterns as int64 (depth > 0.2: the pattern orders like the float)"""
    return depth.contiguous().view(torch.int32).long()


def binning_ref(touched, rect, bits, size):
    """touched [VV, N], rect [VV, N, 4], bits [VV, N] (``depth_bits``) -> a list of VV * grid * grid int64 tensors: for (view, tile) id
    vv * grid^2 + ty * grid + tx the indices of the Gaussians with touched > 0 whose rectangle holds the tile, ordered by
    (depth bits, index)."""
    grid = (size + TILE - 1) // TILE
    ty, tx = torch.arange(grid * grid).div(grid, rounding_mode="floor").view(-1, 1), (torch.arange(grid * grid) % grid).view(-1, 1)
    lists = []
    for vv in range(touched.shape[0]):
        idx = torch.nonzero(touched[vv] > 0).flatten()
        order = idx[torch.argsort(bits[vv][idx], stable=True)]           # stable over ascending indices: ties keep index order
        rc = rect[vv][order].long()
        holds = (rc[:, 0] <= tx) & (tx < rc[:, 2]) & (rc[:, 1] <= ty) & (ty < rc[:, 3])      # [tiles, G]
        lists += [order[holds[t]] for t in range(grid * grid)]
    return lists


def check_binning(lists, touched, ranges, vals_sorted, keys_sorted, n, bits=None, label=""):
    """The kernel's binning against ``binning_ref``'s lists, exactly:  n is the sum of tiles_touched; the ranges of the non-empty tiles
    partition [0, n) in (view, tile) order; empty tiles and views have lo == hi; the first n sorted keys are the tile ids of their ranges
    and do not decrease; every tile's slice of ``vals_sorted`` EQUALS the expected list.  ``keys_sorted``: int64 = the per-view form
    (tile << 32 | depth bits; with ``bits`` [1, N] the low words are checked too), int32 = the batched form ((view, tile) ids)."""
    n, ranges, vals, keys = int(n), ranges.long().cpu().reshape(-1, 2), vals_sorted.long().cpu(), keys_sorted.cpu()
    assert n == int(touched.long().sum()), f"{label}: n = {n}, tiles_touched sums to {int(touched.long().sum())}"
    assert ranges.shape[0] == len(lists), f"{label}: {ranges.shape[0]} ranges for {len(lists)} tiles"
    assert keys.dtype in (torch.int64, torch.int32) and keys.numel() >= n and vals.numel() >= n
    tiles = (keys[:n] >> 32) if keys.dtype == torch.int64 else keys[:n].long()
    assert bool((tiles[1:] >= tiles[:-1]).all()), f"{label}: the sorted keys decrease"
    if keys.dtype == torch.int64 and bits is not None:
        assert torch.equal(keys[:n] & 0xffffffff, bits.reshape(-1)[vals[:n]]), f"{label}: a key's depth word is not its Gaussian's"
    cursor = 0
    for t, want in enumerate(lists):
        lo, hi = int(ranges[t, 0]), int(ranges[t, 1])
        if want.numel() == 0:
            assert lo == hi, f"{label}: empty tile {t} has range [{lo}, {hi})"
            continue
        assert (lo, hi) == (cursor, cursor + want.numel()), f"{label}: tile {t} has range [{lo}, {hi}), expected [{cursor}, {cursor + want.numel()})"
        assert bool((tiles[lo:hi] == t).all()), f"{label}: keys of tile {t}'s range are not {t}"
        assert torch.equal(vals[lo:hi], want), f"{label}: tile {t} holds {vals[lo:hi].tolist()[:12]}..., expected {want.tolist()[:12]}..."
        cursor = hi
    assert cursor == n, f"{label}: the ranges end at {cursor}, n = {n}"


# ---------------------------------------------------------------------------------------------------------------- blend
@torch.no_grad()
def blend_ref(lists, xy, conic_opacity, colours, depth, size, bg, dtype=torch.float64):
    """One view.  ``lists``: its grid * grid per-tile index lists in blend order; xy [N, 2], conic_opacity [N, 4], depth [N] = the kernel's
    fp32 preprocess arrays, colours [N, 3] = the input's.  Per pixel over its tile's list, in ``dtype``:
      power = -0.5 (A dx^2 + C dy^2) - B dx dy ; skipped if power > 0 ; alpha = min(0.99, o e^power) ; skipped if alpha < 1/255 ;
      stop BEFORE the Gaussian that would take T below 1e-4 ; else applied: w = alpha T, T <- T (1 - alpha).
    -> image [3, S, S] (over ``bg``, clamped to [0, 1]), alpha, T, depth = sum w z, median = z of the first applied Gaussian after which
    T < 0.5 (else 0) [S, S]; n_contrib [S, S] = 1-based position in the tile's list of the last applied Gaussian (0: none);
    stopped [S, S] and stop_pos [S, S] = 1-based position of the Gaussian the pixel stopped before (0: none); ambiguous [S, S]: for a Gaussian evaluated up to and including the first stop, alpha 255 within 1e-4 (relative) of 1,
    |power| < 1e-4, or T (1 - alpha) within 1e-4 (relative) of 1e-4; ambiguous_median: T after an applied Gaussian within 1e-4 of 0.5."""
    grid = (size + TILE - 1) // TILE
    assert len(lists) == grid * grid
    xy, co, rgb, z, bg = xy.to(dtype), conic_opacity.to(dtype), colours.to(dtype), depth.to(dtype), torch.as_tensor(bg, dtype=dtype)
    f = lambda dt, v=0: torch.full((size, size), v, dtype=dt)
    out = dict(image=bg.view(3, 1, 1).expand(3, size, size).clamp(0, 1).clone(), alpha=f(dtype), T=f(dtype, 1), depth=f(dtype), median=f(dtype),
               n_contrib=f(torch.int64), stop_pos=f(torch.int64), stopped=f(torch.bool), ambiguous=f(torch.bool), ambiguous_median=f(torch.bool))
    for t, L in enumerate(lists):
        if L.numel() == 0:
            continue
        ty, tx = divmod(t, grid)
        ys, xs = torch.meshgrid(torch.arange(ty * TILE, min(size, ty * TILE + TILE)), torch.arange(tx * TILE, min(size, tx * TILE + TILE)), indexing="ij")
        sh = ys.shape
        ys, xs = ys.reshape(-1, 1), xs.reshape(-1, 1)
        dx, dy = xy[L, 0] - xs.to(dtype), xy[L, 1] - ys.to(dtype)                          # [P, G]
        power = -0.5 * (co[L, 0] * dx * dx + co[L, 2] * dy * dy) - co[L, 1] * dx * dy
        raw = co[L, 3] * torch.exp(power)
        alpha = torch.clamp(raw, max=0.99)
        hit = (power <= 0) & (alpha >= 1.0 / 255.0)
        keep = torch.where(hit, 1.0 - alpha, torch.ones_like(alpha))
        T_before = torch.cat([torch.ones_like(keep[:, :1]), torch.cumprod(keep, dim=1)[:, :-1]], dim=1)
        T_after = T_before * (1.0 - alpha)
        stop = hit & (T_after < 1e-4)
        stops = torch.cumsum(stop.long(), dim=1)
        live = (stops - stop.long()) == 0                                                   # up to and including the first stop
        apply = hit & (stops == 0)
        w = torch.where(apply, alpha * T_before, torch.zeros_like(alpha))
        T_final = torch.where(apply, 1.0 - alpha, torch.ones_like(alpha)).prod(dim=1)
        cross = apply & (T_after < 0.5)
        first = torch.argmax(cross.long(), dim=1)
        m = DECISION_MARGIN
        amb = live & (((raw * 255.0 - 1.0).abs() < m) | (power.abs() < m) | (hit & ((T_after * 1e4 - 1.0).abs() < m)))
        sl = (slice(ty * TILE, ty * TILE + sh[0]), slice(tx * TILE, tx * TILE + sh[1]))
        out["image"][:, sl[0], sl[1]] = (w @ rgb[L] + T_final.unsqueeze(1) * bg).clamp(0, 1).t().reshape(3, *sh)
        out["alpha"][sl] = w.sum(dim=1).view(sh)
        out["T"][sl] = T_final.view(sh)
        out["depth"][sl] = (w * z[L]).sum(dim=1).view(sh)
        out["median"][sl] = torch.where(cross.any(dim=1), z[L][first], torch.zeros_like(T_final)).view(sh)
        out["n_contrib"][sl] = (apply.long() * torch.arange(1, L.numel() + 1)).max(dim=1).values.view(sh)
        out["stopped"][sl] = stop.any(dim=1).view(sh)
        out["stop_pos"][sl] = torch.where(stop.any(dim=1), torch.argmax(stop.long(), dim=1) + 1, torch.zeros_like(first)).view(sh)
        out["ambiguous"][sl] = amb.any(dim=1).view(sh)
        out["ambiguous_median"][sl] = (apply & ((T_after - 0.5).abs() < AMBIGUOUS_MARGIN)).any(dim=1).view(sh)
    return out


def blend_bounds(ref, ref32, z_max):
    """Per-pixel bounds from the reference alone: max(2e-5, 8 x the largest error of the fp32 CPU evaluation ``ref32`` against the fp64
    one ``ref``) over the pixels ambiguous in neither; depth relative to ``z_max``.  -> (bounds, the fp32 evaluation's errors)."""
    ok = ~(ref["ambiguous"] | ref32["ambiguous"])
    scale = dict(image=1.0, alpha=1.0, T=1.0, depth=max(z_max, 1e-30))
    err = {k: float(((ref32[k].double() - ref[k]).abs() / s)[..., ok].max()) if bool(ok.any()) else 0.0 for k, s in scale.items()}
    return {k: max(PIXEL_FLOOR, FP32_FACTOR * e) for k, e in err.items()}, err


def check_blend(ref, bounds, z_max, label="", **got):
    """The kernel's maps of one view against ``blend_ref``, at EVERY pixel that is not ambiguous (no share allowance).  ``got``: any of
    image [3, S, S], alpha, T, depth, median [S, S] (fp32), n_contrib [S, S] (int).  image, alpha, T and depth / z_max are held to
    ``bounds`` per pixel; n_contrib is exact; median is the reference's Gaussian's own fp32 z (exact), away from ``ambiguous_median``
    too.  Prints the figures, asserts the ambiguous share is within the cap, -> the figures."""
    ok = ~ref["ambiguous"]
    fig = dict(ambiguous=float(ref["ambiguous"].double().mean()))
    assert fig["ambiguous"] <= AMBIGUOUS_CAP, f"{label}: {fig['ambiguous']:.3%} of the pixels are ambiguous: a condition of the inputs"
    fails = []
    for k in ("image", "alpha", "T", "depth"):
        if k in got:
            assert bool(torch.isfinite(got[k]).all()), f"{label}: {k} is not finite"
            d = (got[k].double().cpu() - ref[k]).abs() / (max(z_max, 1e-30) if k == "depth" else 1.0)
            fig[k] = float(d[..., ok].max()) if bool(ok.any()) else 0.0
            if fig[k] > bounds[k]:
                fails.append(f"{k}: {fig[k]:.3e} > {bounds[k]:.3e} at {int((d > bounds[k])[..., ok].sum())} pixel values")
    if "n_contrib" in got:
        bad = ok & (got["n_contrib"].long().cpu() != ref["n_contrib"])
        fig["n_contrib_bad"] = int(bad.sum())
        if fig["n_contrib_bad"]:
            fails.append(f"n_contrib differs at {fig['n_contrib_bad']} pixels, first {torch.nonzero(bad)[0].tolist()}")
    if "median" in got:
        okm = ok & ~ref["ambiguous_median"]
        fig["ambiguous_median"] = float((~okm).double().mean())
        assert fig["ambiguous_median"] <= AMBIGUOUS_CAP, f"{label}: {fig['ambiguous_median']:.3%} ambiguous medians"
        bad = okm & (got["median"].float().cpu() != ref["median"].float())
        fig["median_bad"] = int(bad.sum())
        if fig["median_bad"]:
            fails.append(f"median depth is another Gaussian's at {fig['median_bad']} pixels, first {torch.nonzero(bad)[0].tolist()}")
    print(f"gs stages {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    assert not fails, f"{label}: " + "; ".join(fails)
    return fig


ARRAYS = ("depth", "xy", "conic_opacity", "rect", "tiles_touched", "ranges", "keys_sorted", "vals_sorted")


def read_arrays(arrays):
    """``GaussianRenderer.binning`` / ``binning_view`` (views of device buffers the next pass overwrites) -> CPU copies"""
    torch.cuda.synchronize()
    return dict({k: arrays[k].cpu().clone() for k in ARRAYS}, n=arrays["n"])


def check_views_per_pixel(a, gaussians, V, size, bg, label="", **maps):
    """The exact binning rule and the per-pixel blend rule for a whole batched pass: ``a`` = ``read_arrays`` of it, gaussians [B, N, 14]
    (CPU), ``maps`` = the pass's outputs as for ``check_blend`` with a leading dimension B * V.  -> the per-tile lists."""
    bits = depth_bits(a["depth"])
    lists = binning_ref(a["tiles_touched"], a["rect"], bits, size)
    check_binning(lists, a["tiles_touched"], a["ranges"], a["vals_sorted"], a["keys_sorted"], a["n"], bits, label)
    tiles = ((size + TILE - 1) // TILE) ** 2
    for vv in range(a["depth"].shape[0]):
        args = (lists[vv * tiles:(vv + 1) * tiles], a["xy"][vv], a["conic_opacity"][vv], gaussians[vv // V, :, 11:14], a["depth"][vv], size, bg)
        ref, ref32 = blend_ref(*args), blend_ref(*args, dtype=torch.float32)
        m = a["tiles_touched"][vv] > 0
        z_max = float(a["depth"][vv][m].max()) if bool(m.any()) else 1.0
        bounds, _ = blend_bounds(ref, ref32, z_max)
        check_blend(ref, bounds, z_max, f"{label} view {vv}", **{k: x[vv] for k, x in maps.items()})
    return lists


# ---------------------------------------------------------------------------------------------------------------- cases
def _expand(cv, cvp, B):
    return cv.unsqueeze(0).expand(B, -1, -1, -1).contiguous(), cvp.unsqueeze(0).expand(B, -1, -1, -1).contiguous()


def _away(cv, cvp, views, proj):
    """the listed views look AWAY from the scene (tests/test_gs_gpu.py::test_batched_pass_equals_the_per_view_loop): nothing in front"""
    cv, cvp = cv.clone(), cvp.clone()
    for v in views:
        cv[v, :, 2] = -cv[v, :, 2]
        cvp[v] = cv[v] @ proj
    return cv, cvp


def _proj():
    from videomv_amd.gs import GaussianRenderer
    return GaussianRenderer(output_size=16).proj_matrix


# name -> (kind, B, V, N, S, seed).  Each is the smallest shape at which the named thing can go wrong (tests/test_gs_stages_gpu.py lists
# what each pins); the seeds are those for which the cap conditions and the table conditions hold (tests/test_gs_stages_cpu.py).
CASES = {
    "plain": ("plain", 1, 3, 300, 64, 1),
    "partial-40": ("plain", 2, 2, 200, 40, 2), "partial-50": ("plain", 1, 1, 200, 50, 3),
    "dup-256": ("plain", 1, 2, 128, 32, 4), "dup-257": ("plain", 1, 1, 257, 32, 5), "dup-255": ("plain", 1, 3, 85, 32, 6),
    "dup-span": ("plain", 1, 3, 100, 32, 7),
    "rounds": ("rounds", 1, 2, 64, 272, 8),
    "ties": ("ties", 1, 2, 96, 48, 9),
    "empty-views": ("empty", 1, 4, 100, 32, 10),
    "bits-17": ("plain", 1, 17, 40, 16, 11), "bits-32": ("plain", 1, 2, 60, 64, 12), "bits-1": ("plain", 1, 1, 40, 16, 13),
    "bits-9": ("plain", 1, 1, 60, 48, 14),
    "deep-900": ("deep", 1, 1, 900, 32, 7), "deep-511": ("deep", 1, 1, 511, 32, 7), "deep-512": ("deep", 1, 1, 512, 32, 7),
    "deep-513": ("deep", 1, 1, 513, 32, 7),
    "stop": ("stop", 1, 2, 200, 32, 6),
}


def build_case(name):
    """-> (gaussians [B, N, 14], cam_view [B, V, 4, 4], cam_view_proj [B, V, 4, 4], size), fp32"""
    kind, B, V, N, S, seed = CASES[name]
    cv, cvp = _cams(V)
    if kind == "deep":
        # gs_depth_ref.staging_scene: identity camera, one tile that holds every Gaussian.  Screen sigma 0.5 px, not its default 0.6: at
        # 0.6 the radius before the ceil is 2.96 .. 3.02 and 3.4 % of the records are boundary records whatever the seed; at 0.5 it is 2.8
        return (staging_scene(size=S, n=N, seed=seed, sigma_px=0.5).unsqueeze(0), torch.eye(4).view(1, 1, 4, 4),
                _proj().view(1, 1, 4, 4).clone(), S)
    if kind == "stop":                       # the dense, opaque cluster of tests/test_gs_fit_gpu.py
        g = _scene(N, seed, spread=0.15, scale=(0.05, 0.12), opacity=(0.6, 0.95)).unsqueeze(0)
    elif kind == "rounds":
        # 24 Gaussians wide enough for more than 256 of the 289 tiles, between 40 records above every orbit camera and behind it
        # (y = 20 .. 50: view depth < 0 at elevation 15 deg), the first and the last record among them
        gen = torch.Generator().manual_seed(seed)
        g = _scene(N, seed, spread=0.2, scale=(0.2, 0.4), opacity=(0.2, 0.8))
        culled = torch.ones(N, dtype=torch.bool)
        culled[torch.arange(24) * 5 // 2 + 2] = False                     # 2, 4, 7, 9, ... 59: never index 0 or 63
        g[culled, 1] = 20.0 + 30.0 * torch.rand(int(culled.sum()), generator=gen)
        g = g.unsqueeze(0)
    elif kind == "ties":                     # 32 positions, each used by indices i, i + 32, i + 64 with their own colour, opacity, scale
        g = _scene(N, seed)
        g[:, 0:3] = g[:32, 0:3].repeat(3, 1)
        g = g.unsqueeze(0)
    else:
        g = torch.stack([_scene(N, seed + 100 * b) for b in range(B)])
    if kind == "empty":
        cv, cvp = _away(cv, cvp, (1, 3), _proj())
    cv, cvp = _expand(cv, cvp, B)
    if B > 1:                                # the second sample sees its own Gaussians from the cameras in the other order
        cv[1], cvp[1] = cv[0].flip(0), cvp[0].flip(0)
    return g, cv, cvp, S
