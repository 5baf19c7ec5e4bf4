"""The stage-wise rasteriser reference (tests/gs_stage_ref.py) without a GPU: its comparators accept arrays simulated with the fp32
oracle and a few lines of Python binning for every case of tests/test_gs_stages_gpu.py; the conditions its caps rest on hold for the
chosen seeds; each small fault a hand-written stage could produce is rejected by the matching comparator — and the image-level bound
of tests/test_gs_gpu.py (mean |error| < 2e-4, fewer than 0.2 % of the pixels off by more than 2e-3) accepts a lost instance and a
swapped pair on its own 1500 / 128 scene, which is why the stage tests exist."""
import functools

import pytest
import torch

from oracle.gs_ref import preprocess, render as oracle_render
from tests import gs_stage_ref as R
from tests.gs_depth_ref import AMBIGUOUS_CAP, blend_depth
from tests.test_gs_gpu import _cams as _gs_cams, _scene as _gs_scene

TILE = 16


def simulate(g, view, view_proj, size, vv=0):
    """What the kernels leave on the device for one view, from the fp32 oracle: the preprocess arrays, and the binning by a plain Python
    sort of (tile, depth bits, index) triples — in both key forms (``vv`` = the view's number in the batched one)."""
    pp = preprocess(g[:, 0:3], g[:, 4:7], g[:, 7:11], view.float(), view_proj.float(), size, R.TAN)
    grid = (size + TILE - 1) // TILE
    rect = pp["rect"].int()
    touched = torch.where(pp["valid"], (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]), torch.zeros_like(rect[:, 0]))
    depth = pp["depth"].float()
    bits = R.depth_bits(depth)
    inst = sorted((y * grid + x, int(bits[i]), i) for i in torch.nonzero(touched).flatten().tolist()
                  for y in range(int(rect[i, 1]), int(rect[i, 3])) for x in range(int(rect[i, 0]), int(rect[i, 2])))
    ranges = torch.zeros(grid * grid, 2, dtype=torch.int32)
    for j, (t, _, _) in enumerate(inst):
        if j == 0 or inst[j - 1][0] != t:
            ranges[t, 0] = j
        ranges[t, 1] = j + 1
    return dict(touched=touched, rect=rect, depth=depth, bits=bits, xy=pp["xy"].float(), valid=pp["valid"],
                co=torch.cat([pp["conic"].float(), g[:, 3:4].float()], dim=1), n=len(inst), ranges=ranges,
                vals=torch.tensor([i for _, _, i in inst], dtype=torch.int32),
                keys64=torch.tensor([(t << 32) | b for t, b, _ in inst], dtype=torch.int64),
                keys32=torch.tensor([vv * grid * grid + t for t, _, _ in inst], dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def _case(name):
    """every view of a case: (sample's Gaussians, fp64 preprocess reference, simulated arrays, expected lists, fp64 blend)"""
    g, cv, cvp, S = R.build_case(name)
    views = []
    for b in range(g.shape[0]):
        for v in range(cv.shape[1]):
            ref = R.preprocess_ref(g[b], cv[b, v], cvp[b, v], S)
            sim = simulate(g[b], cv[b, v], cvp[b, v], S, vv=b * cv.shape[1] + v)
            lists = R.binning_ref(sim["touched"][None], sim["rect"][None], sim["bits"][None], S)
            views.append((g[b], ref, sim, lists, R.blend_ref(lists, sim["xy"], sim["co"], g[b, :, 11:14], sim["depth"], S, R.BG)))
    return S, views


@pytest.mark.parametrize("name", list(R.CASES))
def test_comparators_accept_the_simulated_arrays_and_the_caps_hold(name):
    S, views = _case(name)
    grid = (S + TILE - 1) // TILE
    boundary = sum(int(ref["boundary"].sum()) for _, ref, *_ in views) / sum(ref["boundary"].numel() for _, ref, *_ in views)
    assert boundary <= R.BOUNDARY_CAP, boundary
    for vv, (g, ref, sim, lists, blend) in enumerate(views):
        R.check_preprocess(ref, sim["touched"], sim["rect"], S, f"{name} view {vv}")
        err = R.preprocess_errors(ref, sim["depth"], sim["xy"], sim["co"][:, :3], sim["valid"] & ref["valid"])
        assert err["xy"] < 1e-3 and err["conic"] < 1e-3 and err["depth"] < 1e-5, err
        R.check_binning(lists, sim["touched"], sim["ranges"], sim["vals"], sim["keys64"], sim["n"], sim["bits"][None], name)
        off = vv * grid * grid                                            # the batched form: this view's tiles behind vv empty views
        R.check_binning([torch.zeros(0, dtype=torch.int64)] * off + lists, sim["touched"],
                        torch.cat([torch.zeros(off, 2, dtype=torch.int32), sim["ranges"]]), sim["vals"], sim["keys32"], sim["n"], None, name)
        assert float(blend["ambiguous"].double().mean()) <= AMBIGUOUS_CAP and float(blend["ambiguous_median"].double().mean()) <= AMBIGUOUS_CAP
        blend32 = R.blend_ref(lists, sim["xy"], sim["co"], g[:, 11:14], sim["depth"], S, R.BG, dtype=torch.float32)
        z_max = float(sim["depth"][sim["valid"]].max()) if bool(sim["valid"].any()) else 1.0
        bounds, _ = R.blend_bounds(blend, blend32, z_max)
        got = {k: blend32[k] for k in ("image", "alpha", "T", "depth", "n_contrib", "median")}
        got["n_contrib"] = torch.where(blend32["ambiguous"], blend["n_contrib"], got["n_contrib"])   # (a pixel ambiguous in fp32 only)
        got["median"] = torch.where(blend32["ambiguous"] | blend32["ambiguous_median"], blend["median"].float(), got["median"])
        R.check_blend(blend, bounds, z_max, f"{name} view {vv} (fp32 CPU evaluation)", **got)


def test_table_conditions():
    """what the cases of tests/test_gs_stages_gpu.py are named for, from the fp32 oracle for the chosen seeds"""
    _, views = _case("rounds")
    for _, _, sim, _, _ in views:
        t = sim["touched"]
        assert int((t > 256).sum()) >= 8 and int(t[0]) == 0 and int(t[-1]) == 0 and int((t == 0).sum()) == 40, t
    _, views = _case("ties")
    for _, _, sim, lists, _ in views:
        assert any(L.numel() > 1 and bool((sim["bits"][L][1:] == sim["bits"][L][:-1]).any()) for L in lists)
    for name, n in (("deep-900", 768), ("deep-511", 510), ("deep-512", 511), ("deep-513", 512)):
        _, views = _case(name)
        assert max(L.numel() for L in views[0][3]) > n, name
    assert [max(L.numel() for L in _case(k)[1][0][3]) for k in ("deep-511", "deep-512", "deep-513")] == [511, 512, 513]
    _, views = _case("stop")
    for _, _, _, _, blend in views:
        st = blend["stopped"]
        assert int(st.sum()) > 20
    for name in ("partial-40", "partial-50"):
        S, views = _case(name)
        grid = (S + TILE - 1) // TILE
        for _, _, sim, lists, blend in views:
            rc = sim["rect"][sim["touched"] > 0]
            assert bool((rc[:, 2] == grid).any()) and bool((rc[:, 3] == grid).any())
            assert bool((blend["alpha"][:, (grid - 1) * TILE:] > 0.05).any()) and bool((blend["alpha"][(grid - 1) * TILE:] > 0.05).any())
    _, views = _case("empty-views")
    assert [sim["n"] > 0 for _, _, sim, _, _ in views] == [True, False, True, False]
    for name, tiles in (("bits-17", 17), ("bits-32", 32), ("bits-1", 1), ("bits-9", 9)):
        S, views = _case(name)
        assert len(views) * ((S + TILE - 1) // TILE) ** 2 == tiles and views[-1][3][-1].numel() > 0, name      # the highest tile id is in use


def _rejects(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def _binning_args(sim, lists, **change):
    a = dict(lists=lists, touched=sim["touched"], ranges=sim["ranges"], vals=sim["vals"], keys=sim["keys64"], n=sim["n"], bits=sim["bits"][None])
    a.update(change)
    return a["lists"], a["touched"], a["ranges"], a["vals"], a["keys"], a["n"], a["bits"]


def _drop(sim, j):
    """instance j removed from the sorted arrays, the ranges behind it moved up"""
    t = int(sim["keys64"][j] >> 32)
    keep = torch.arange(sim["n"]) != j
    ranges = sim["ranges"].clone()
    ranges[t, 1] -= 1
    later = (ranges[:, 0] > j) & (ranges[:, 1] > ranges[:, 0])
    ranges[later] -= 1
    return dict(vals=sim["vals"][keep], keys=sim["keys64"][keep], n=sim["n"] - 1, ranges=ranges)


def _swap(sim, j):
    vals, keys = sim["vals"].clone(), sim["keys64"].clone()
    vals[[j, j + 1]], keys[[j, j + 1]] = vals[[j + 1, j]], keys[[j + 1, j]]
    return dict(vals=vals, keys=keys)


def test_teeth_every_small_fault_is_rejected():
    _, views = _case("plain")
    g, ref, sim, lists, blend = views[0]
    longest = max(range(len(lists)), key=lambda t: lists[t].numel())
    lo = int(sim["ranges"][longest, 0])
    R.check_binning(*_binning_args(sim, lists))
    # one instance removed from one tile's list
    _rejects(R.check_binning, *_binning_args(sim, lists, **_drop(sim, lo + 3)))
    # one adjacent pair of a list swapped (keys with them, and the values alone)
    _rejects(R.check_binning, *_binning_args(sim, lists, **_swap(sim, lo + 3)))
    _rejects(R.check_binning, *_binning_args(sim, lists, vals=_swap(sim, lo + 3)["vals"]))
    # the last tile id's range emptied
    last = max(t for t in range(len(lists)) if lists[t].numel())
    ranges = sim["ranges"].clone()
    ranges[last] = 0
    _rejects(R.check_binning, *_binning_args(sim, lists, ranges=ranges))
    # one tie resolved by descending index
    _, tviews = _case("ties")
    _, _, tsim, tlists, _ = tviews[0]
    R.check_binning(*_binning_args(tsim, tlists))
    j = next(j for j in range(tsim["n"] - 1) if int(tsim["keys64"][j]) == int(tsim["keys64"][j + 1]))
    _rejects(R.check_binning, *_binning_args(tsim, tlists, **_swap(tsim, j)))
    # radius one short on one Gaussian: one whose rectangle shrinks with it, away from the boundary records
    grid = 4
    for i in torch.nonzero(ref["valid"] & ~ref["boundary"]).flatten().tolist():
        x, y, r = float(ref["xy"][i, 0]), float(ref["xy"][i, 1]), float(ref["radius"][i]) - 1
        c = lambda v: max(0, min(grid, int(v // TILE)))
        short = [c(x - r), c(y - r), c(x + r + 15), c(y + r + 15)]
        if short != ref["rect"][i].tolist():
            break
    rect, touched = sim["rect"].clone(), sim["touched"].clone()
    rect[i] = torch.tensor(short, dtype=torch.int32)
    touched[i] = (short[2] - short[0]) * (short[3] - short[1])
    R.check_preprocess(ref, sim["touched"], sim["rect"], 64)
    _rejects(R.check_preprocess, ref, touched, rect, 64)
    # one pad pixel: one colour value off by 1e-3 at one pixel
    z_max = float(sim["depth"][sim["valid"]].max())
    bounds, _ = R.blend_bounds(blend, R.blend_ref(lists, sim["xy"], sim["co"], g[:, 11:14], sim["depth"], 64, R.BG, dtype=torch.float32), z_max)
    assert bounds["image"] == R.PIXEL_FLOOR                                   # the floor binds (fp32 CPU evaluation: a few 1e-7)
    image = blend["image"].float()
    R.check_blend(blend, bounds, z_max, "intact", image=image, n_contrib=blend["n_contrib"], median=blend["median"].float())
    py, px = (int(v) for v in torch.nonzero(~blend["ambiguous"] & (blend["alpha"] > 0.2))[0])
    image[1, py, px] += 1e-3 if image[1, py, px] < 0.5 else -1e-3
    _rejects(lambda: R.check_blend(blend, bounds, z_max, "pad", image=image))
    n_contrib = blend["n_contrib"].clone()
    n_contrib[py, px] -= 1
    _rejects(lambda: R.check_blend(blend, bounds, z_max, "count", n_contrib=n_contrib))


def test_the_image_bound_accepts_a_lost_instance_and_a_swapped_pair():
    """The 1500 / 128 scene of tests/test_gs_gpu.py::test_rasteriser_matches_oracle, view 0, the longest tile list: the deepest
    instance that any pixel of the tile still blends lost, and an adjacent pair about halfway to it swapped.  The image the faulty lists blend to is within that test's bound
    of the intact one, so the image test passes both; ``check_binning`` rejects both."""
    g = _gs_scene(1500, 2, True)
    cv, cvp = _gs_cams(3)
    S = 128
    sim = simulate(g, cv[0], cvp[0], S)
    lists = R.binning_ref(sim["touched"][None], sim["rect"][None], sim["bits"][None], S)
    R.check_binning(*_binning_args(sim, lists))
    intact = R.blend_ref(lists, sim["xy"], sim["co"], g[:, 11:14], sim["depth"], S, (0.5, 0.5, 0.5))
    longest = max(range(len(lists)), key=lambda t: lists[t].numel())
    lo, hi = (int(v) for v in sim["ranges"][longest])
    ty, tx = divmod(longest, S // TILE)
    seen = int(intact["n_contrib"][ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].max())      # the deepest instance a pixel still blends
    assert 2 < seen <= hi - lo
    # (a swapped pair shows only where both Gaussians reach the same pixel: the first such pair from halfway on, this tile blended alone)
    none = [torch.zeros(0, dtype=torch.int64)] * len(lists)
    alone = lambda L: R.blend_ref(none[:longest] + [L] + none[longest + 1:], sim["xy"], sim["co"], g[:, 11:14], sim["depth"], S, (0.5, 0.5, 0.5))["image"]
    L0, base = lists[longest], alone(lists[longest])
    pair = next(j for j in range(seen // 2, seen - 1)
                if float((alone(torch.cat([L0[:j], L0[j + 1:j + 2], L0[j:j + 1], L0[j + 2:]])) - base).abs().max()) > 0)
    for label, fault in (("drop", _drop(sim, lo + seen - 1)), ("swap", _swap(sim, lo + pair))):
        _rejects(R.check_binning, *_binning_args(sim, lists, **fault))
        ranges, vals = fault.get("ranges", sim["ranges"]), fault["vals"].long()
        faulty = R.blend_ref([vals[int(a):int(b)] for a, b in ranges], sim["xy"], sim["co"], g[:, 11:14], sim["depth"], S, (0.5, 0.5, 0.5))
        for k in ("image", "alpha"):
            d = (faulty[k] - intact[k]).abs()
            print(f"{label} {k}: mean {float(d.mean()):.3e}, share > 2e-3 {float((d > 2e-3).double().mean()):.3e}, max {float(d.max()):.3e}")
            assert float(d.mean()) < 2e-4 and float((d > 2e-3).double().mean()) < 2e-3
        assert float((faulty["image"] - intact["image"]).abs().max()) > 0      # (the fault is in the image, below the bound)


def test_blend_reference_agrees_with_the_oracle_and_the_depth_reference():
    """same rules as oracle.gs_ref.render (fp32) and gs_depth_ref.blend_depth (fp64 blend) on the plain case: image and alpha within 1e-6
    of the latter, within fp32 rounding of the former, and the same medians"""
    _, views = _case("plain")
    g, _, sim, lists, blend = views[1]
    gc, cv, cvp, S = R.build_case("plain")
    bg = torch.tensor(R.BG)
    ref = blend_depth(g, cv[0, 1], cvp[0, 1], S, R.TAN, bg)
    assert float((blend["image"] - ref["image"].clamp(0, 1)).abs().max()) < 1e-6 and float((blend["alpha"] - ref["alpha"]).abs().max()) < 1e-6
    assert float((blend["depth"] - ref["D"]).abs().max()) < 1e-6 and float((blend["T"] - (1 - ref["alpha"])).abs().max()) < 1e-6
    clear = ~blend["ambiguous_median"]
    assert float((blend["median"] - ref["median"]).abs()[clear].max()) < 1e-6 and bool(((blend["median"] > 0) == ref["has"])[clear].all())
    img, alpha, D = oracle_render(g[:, 0:3], g[:, 3:4], g[:, 4:7], g[:, 7:11], g[:, 11:14], cv[0, 1], cvp[0, 1], S, R.TAN, bg)
    ok = ~blend["ambiguous"]
    assert float((img.clamp(0, 1).double() - blend["image"]).abs()[:, ok].max()) < 1e-5
    assert float((alpha[0].double() - blend["alpha"]).abs()[ok].max()) < 1e-5 and float((D[0].double() - blend["depth"]).abs()[ok].max()) < 2e-5
