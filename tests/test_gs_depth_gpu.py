"""The rasteriser's depth mode (csrc/raster.hip gs_render_batch_kernel<false, true> through vmv_gs_batch_render_depth and
GaussianRenderer.render_depth) on the device: expected depth against the splatting oracle, median depth against the fp64 restatement
of tests/gs_depth_ref.py (checked on the CPU in tests/test_gs_depth_cpu.py), staging past one LDS batch, the edges, batch independence,
the store footprint, a closed form and the entrance keys.  Bounds are in ``gs_depth_ref.compare_view``."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle.gs_ref import render as oracle_render
from tests import footprint as FP
from tests import gs_stage_ref as R
from tests.gs_depth_ref import blend_depth, blend_depth_views, compare_view, staging_scene
from tests.test_gs_gpu import _cams, _scene

pytestmark = pytest.mark.gpu

FOVY = 39.6
TAN = math.tan(0.5 * math.radians(FOVY))
BG = (0.5, 0.5, 0.5)
SCENES = [(3000, 64, False, 1), (1500, 128, True, 2), (300, 64, False, 4)]


@functools.lru_cache(maxsize=None)
def _reference(n, size, big, seed):
    """scene, cameras and the fp64 reference of every view: computed once, shared, never modified"""
    g = _scene(n, seed, big)
    cv, cvp = _cams(3)
    return g, cv, cvp, blend_depth_views(g, cv, cvp, size, FOVY, torch.tensor(BG))


@functools.lru_cache(maxsize=None)
def _rendered(n, size, big, seed):
    from videomv_amd.gs import GaussianRenderer
    g, cv, cvp, _ = _reference(n, size, big, seed)
    r = GaussianRenderer(output_size=size)
    args = (g.cuda().unsqueeze(0), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None)
    out = r.render_depth(*args, bg_color=torch.tensor(BG).cuda())
    plain = r.render(*args, bg_color=torch.tensor(BG).cuda())
    torch.cuda.synchronize()
    arrays = R.read_arrays(r.binning(1, 3, n, args[0].device))          # what the pass left on the device (the two passes: the same bits)
    return {k: v.cpu() for k, v in out.items()}, {k: v.cpu() for k, v in plain.items()}, arrays


@pytest.mark.parametrize("n,size,big,seed", SCENES)
def test_expected_depth_matches_the_oracle(n, size, big, seed):
    """depth / z_max is a colour channel with values in (0, 1] — the same weighted sum — so it is held to the rasteriser's colour bound
    against the oracle's third return value; image and alpha are render()'s bits."""
    g, cv, cvp, refs = _reference(n, size, big, seed)
    out, plain, _ = _rendered(n, size, big, seed)
    assert out["depth"].shape == out["median_depth"].shape == (1, 3, 1, size, size) and out["depth"].dtype == torch.float32
    assert torch.equal(out["image"], plain["image"]) and torch.equal(out["alpha"], plain["alpha"])
    for v in range(3):
        _, _, D = oracle_render(g[:, 0:3], g[:, 3:4], g[:, 4:7], g[:, 7:11], g[:, 11:14], cv[v], cvp[v], size, TAN, torch.tensor(BG))
        d = (out["depth"][0, v, 0] - D[0]).abs() / refs[v]["z_max"]
        print(f"expected depth vs oracle, view {v}: mean {float(d.mean()):.3e}, off {float((d > 2e-3).float().mean()):.3e}")
        assert float(d.mean()) < 2e-4, float(d.mean())
        assert float((d > 2e-3).float().mean()) < 2e-3, float((d > 2e-3).float().mean())


@pytest.mark.parametrize("n,size,big,seed", SCENES)
def test_median_depth_matches_the_reference(n, size, big, seed):
    g, _, _, refs = _reference(n, size, big, seed)
    out, _, arrays = _rendered(n, size, big, seed)
    for v in range(3):
        fig = compare_view(out["depth"][0, v, 0], out["median_depth"][0, v, 0], refs[v], f"scene {seed} view {v}")
        if n == 300:              # the sparse scene shows both branches: pixels with a median and pixels without
            assert 0.17 <= fig["with_median"] <= 0.20, fig
            assert bool(refs[v]["has"].any()) and bool((~refs[v]["has"]).any())
            assert bool((out["median_depth"][0, v, 0] > 0).any()) and bool((out["median_depth"][0, v, 0] == 0).any())
    if n == 300:
        # beside compare_view's statistical bounds: this pass's binning exact, and at every non-ambiguous pixel the median the reference's
        # own Gaussian and image, alpha and expected depth within the per-pixel bound of tests/gs_stage_ref.py
        R.check_views_per_pixel(arrays, g.unsqueeze(0), 3, size, BG, f"depth scene {seed}", image=out["image"][0], alpha=out["alpha"][0, :, 0],
                                depth=out["depth"][0, :, 0], median=out["median_depth"][0, :, 0])


def _identity_render(g, size, bg=(0.0, 0.0, 0.0)):
    from videomv_amd.gs import GaussianRenderer
    r = GaussianRenderer(output_size=size)
    out = r.render_depth(g.cuda().unsqueeze(0), torch.eye(4).view(1, 1, 4, 4).cuda(), r.proj_matrix.view(1, 1, 4, 4).cuda(), None,
                         bg_color=torch.tensor(bg).cuda())
    torch.cuda.synchronize()
    return r, {k: v.cpu() for k, v in out.items()}


def test_staging_beyond_one_batch():
    """One tile with more than 512 instances (three LDS batches of 256 and a tail) and medians that cross deep in the list — asserted
    from the reference — so a stale or mis-indexed z in LDS shows in both outputs."""
    g = staging_scene()
    r, out = _identity_render(g, 32)
    ref = blend_depth(g, torch.eye(4), r.proj_matrix, 32, r.tan_half_fov)
    clear = ref["has"] & (ref["margin"] >= 1e-4)
    assert int(ref["count"].max()) > 512
    assert int((clear & (ref["pos"] >= 256)).sum()) > 0 and int((clear & (ref["pos"] >= 512)).sum()) > 0
    compare_view(out["depth"][0, 0, 0], out["median_depth"][0, 0, 0], ref, "staging")
    late = clear & (ref["pos"] >= 256)                                 # and those pixels themselves, one by one
    assert float((out["median_depth"][0, 0, 0].double()[late] - ref["median"][late]).abs().max()) <= 1e-5 * ref["z_max"]


def test_edges_partial_tiles_odd_counts_and_an_empty_view():
    from videomv_amd.gs import GaussianRenderer
    size = 40                                                          # 2.5 tiles: lanes outside the image in the last row / column
    g = _scene(301, 8)
    cv, cvp = _cams(2)
    away = cv[1].clone()                                               # view 1 looks away: it sees nothing
    away[:, 2] = -away[:, 2]
    r = GaussianRenderer(output_size=size)
    cv, cvp = torch.stack([cv[0], away]), torch.stack([cvp[0], away @ r.proj_matrix])
    bg = torch.tensor([0.2, 0.4, 0.6])
    out = r.render_depth(g.cuda().unsqueeze(0), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None, bg_color=bg.cuda())
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    ref = blend_depth(g, cv[0], cvp[0], size, TAN, bg)
    odd = (ref["count"] % 2 == 1) & ref["has"] & (ref["margin"] >= 1e-4)       # a pad Gaussian (z = 0, weight 0) closes the last pair
    assert bool(odd.any()) and bool((ref["count"] % 2 == 0).any()) and bool(ref["has"][:, 32:].any()) and bool(ref["has"][32:].any())
    compare_view(out["depth"][0, 0, 0], out["median_depth"][0, 0, 0], ref, "size 40")
    assert float((out["image"][0, 0].double() - ref["image"].clamp(0, 1)).abs().mean()) < 2e-4
    assert float(out["depth"][0, 1].abs().max()) == 0.0 and float(out["median_depth"][0, 1].abs().max()) == 0.0
    assert torch.equal(out["image"][0, 1], bg.view(3, 1, 1).expand(3, size, size)) and float(out["alpha"][0, 1].abs().max()) == 0.0
    # a single Gaussian: the tile's list is [Gaussian, pad]
    one = torch.tensor([[0.0, 0.0, 1.5, 0.8, 0.05, 0.05, 0.05, 1.0, 0.0, 0.0, 0.0, 0.9, 0.2, 0.1]])
    _, o1 = _identity_render(one, size)
    a = o1["alpha"][0, 0, 0]
    assert float(a.max()) > 0.5 and float((o1["depth"][0, 0, 0] - 1.5 * a).abs().max()) < 1e-6
    assert torch.equal(o1["median_depth"][0, 0, 0] > 0, a > 0.5) and float(o1["median_depth"].max()) == 1.5


def test_batch_independence(monkeypatch):
    """B = 2, V = 3 in one call = the six B = V = 1 calls, bit for bit in all four outputs; and a call split by the instance budget"""
    from videomv_amd.gs import GaussianRenderer
    size = 48
    gauss = torch.stack([_scene(900, 31), _scene(900, 32, big=True)]).cuda()
    cv, cvp = _cams(3)
    cv2, cvp2 = torch.stack([cv, cv.flip(0)]).cuda(), torch.stack([cvp, cvp.flip(0)]).cuda()
    bg = torch.tensor([0.1, 0.6, 0.3]).cuda()
    r = GaussianRenderer(output_size=size)
    out = r.render_depth(gauss, cv2, cvp2, None, bg_color=bg)
    total = sum(r.last_num_rendered)
    assert len(r.last_num_rendered) == 1 and float(out["median_depth"].max()) > 0.5
    per_view = []
    for b in range(2):
        for v in range(3):
            one = r.render_depth(gauss[b:b + 1], cv2[b:b + 1, v:v + 1].contiguous(), cvp2[b:b + 1, v:v + 1].contiguous(), None, bg_color=bg)
            per_view += r.last_num_rendered
            for k in ("image", "alpha", "depth", "median_depth"):
                assert torch.equal(one[k][0, 0], out[k][b, v]), (k, b, v)
    assert sum(per_view) == total and min(per_view) > 0
    monkeypatch.setenv("VMV_GS_BATCH_MAX_INSTANCES", str(max(per_view)))             # any one view fits, the larger sample's three do not
    split = r.render_depth(gauss, cv2, cvp2, None, bg_color=bg)
    assert len(r.last_num_rendered) > 2 and sum(r.last_num_rendered) == total
    assert all(torch.equal(split[k], out[k]) for k in out)
    monkeypatch.setenv("VMV_GS_BATCH_MAX_INSTANCES", "1")                             # not even one view fits: no per-view depth mode
    with pytest.raises(NotImplementedError, match="VMV_GS_BATCH_MAX_INSTANCES"):
        r.render_depth(gauss, cv2, cvp2, None, bg_color=bg)
    torch.cuda.synchronize()


def test_store_footprint_and_optional_median():
    """out_depth / out_median_depth inside larger buffers: the guard words before and after are the bits they were; with
    out_median_depth = NULL the call runs and out_depth is unchanged."""
    from videomv_amd.gs import GaussianRenderer
    size, V = 40, 2
    g = _scene(500, 9).cuda().unsqueeze(0)
    cv, cvp = _cams(V)
    cv, cvp = cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda()
    r = GaussianRenderer(output_size=size)
    arenas = {k: FP.Arena(V * size, size, kind="f32") for k in ("depth", "median", "depth_only")}
    bufs = {k: a.buf.clone().cuda() for k, a in arenas.items()}
    pay = {k: a.payload(bufs[k]) for k, a in arenas.items()}
    assert all(p.is_contiguous() and p.data_ptr() == arenas[k].ptr(bufs[k]) for k, p in pay.items())
    bg, (images, alphas) = r._begin(g, cv, torch.tensor(BG), (3, 1))
    assert r._render_batch(g, cv, cvp, bg, images, alphas, pay["depth"], pay["median"])
    assert r._render_batch(g, cv, cvp, bg, images, alphas, pay["depth_only"], None)
    torch.cuda.synchronize()
    for k, a in arenas.items():
        assert FP.stray_report(k, a, bufs[k]) == ""
    assert torch.equal(pay["depth"], pay["depth_only"]) and float(pay["depth"].max()) > 0.5 and float(pay["median"].max()) > 0.5
    full = r.render_depth(g, cv, cvp, None, bg_color=torch.tensor(BG).cuda())
    assert torch.equal(full["depth"].reshape(V * size, size), pay["depth"]) and torch.equal(full["median_depth"].reshape(V * size, size), pay["median"])


def test_closed_form_single_gaussian():
    """the isotropic Gaussian of test_rasteriser_degenerate_scenes (d = 1.5, centre pixel): depth = 1.5 alpha, median 1.5 at o = 0.8
    (alpha = 0.79 > 0.5) and 0 at o = 0.4; the centre pixel's median unprojects to the Gaussian within one pixel footprint."""
    from videomv_amd.gs import depth_to_points
    S, d, s = 64, 1.5, 0.05
    f = S / (2 * TAN)
    var = (f * s / d) ** 2 + 0.3
    for o, median in ((0.8, d), (0.4, 0.0)):
        one = torch.tensor([[0.0, 0.0, d, o, s, s, s, 1.0, 0.0, 0.0, 0.0, 0.9, 0.2, 0.1]])
        r, out = _identity_render(one, S)
        a_centre = o * math.exp(-0.5 * (0.5 ** 2 + 0.5 ** 2) / var)
        assert abs(float(out["alpha"][0, 0, 0, 32, 32]) - a_centre) < 1e-5
        assert abs(float(out["depth"][0, 0, 0, 32, 32]) - d * a_centre) < 1e-5
        assert float(out["median_depth"][0, 0, 0, 32, 32]) == median and float(out["median_depth"].max()) == median
    _, out = _identity_render(torch.tensor([[0.0, 0.0, d, 0.8, s, s, s, 1.0, 0.0, 0.0, 0.0, 0.9, 0.2, 0.1]]), S)
    centre = torch.zeros(S, S, dtype=torch.bool)
    centre[32, 32] = True
    pts, idx = depth_to_points(out["median_depth"][0, 0, 0], torch.eye(4), TAN, mask=centre)
    assert idx.tolist() == [32 * S + 32]
    assert float((pts[0] - torch.tensor([0.0, 0.0, d])).abs().max()) <= 2 * d * TAN / S


def _entrance_cfg(tmp_path, extra):
    from videomv_amd.config import Config
    tmp_path.mkdir(parents=True, exist_ok=True)
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("a wooden chair\na red apple\n")
    argv = ["--cfg", "configs/t2v_infer.yaml", "--debug", "allow_random_init", "True", "num_views", "4",
            "ddim_timesteps", "2", "test_list_path", str(prompts), "log_dir", str(tmp_path / "out"),
            "UNet.num_heads", "2", "UNet.num_res_blocks", "1", "UNet.dim_mult", "[1]", "test_model", "none.pth"] + extra
    cu = Config(load=True, argv=argv)
    cu.cfg_dict["UNet"]["dim"] = 64
    cu.cfg_dict["UNet"]["attn_scales"] = [1.0]
    cu.cfg_dict["resolution"] = [64, 64]
    cu.cfg_dict["lgm_opt"] = dict(down_channels=(32, 64), down_attention=(False, True), mid_attention=True,
                                  up_channels=(64, 32), up_attention=(True, False), num_heads=2, input_size=64,
                                  splat_size=64, output_size=128)
    cu.cfg_dict["auto_encoder"] = {"type": "AutoencoderKL", "embed_dim": 4, "pretrained": "none.pth",
                                   "ddconfig": {"double_z": True, "z_channels": 4, "resolution": 64, "in_channels": 3,
                                                "out_ch": 3, "ch": 32, "ch_mult": [1, 2, 4, 4], "num_res_blocks": 2,
                                                "attn_resolutions": [], "dropout": 0.0}}
    return cu


def test_t2v_entrance_exports_depth_maps_and_points(tmp_path):
    """Two prompts with 8 orbit views, gs_orbit_depth and gs_points: the files of each prompt are written, the depth maps are finite and
    non-negative, the point cloud loads, and the latents are the bits of the run without the keys."""
    from videomv_amd.registry import INFER_ENGINE
    from videomv_amd.gs import load_points_ply
    import videomv_amd.entrance  # noqa: F401
    runs = {}
    for name, extra in (("plain", []), ("export", ["save_gaussians", "True", "gs_orbit_views", "8", "gs_orbit_depth", "True", "gs_points", "True"])):
        cu = _entrance_cfg(tmp_path / name, extra)
        runs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    cfg = runs["export"]
    assert len(cfg.gs_exports) == 2
    for e in cfg.gs_exports:
        d = np.load(e["orbit_depth"])
        assert d.shape == (8, 128, 128) and d.dtype == np.float32 and np.isfinite(d).all() and (d >= 0).all()
        assert os.path.exists(e["orbit_depth_sheet"]) and os.path.exists(e["orbit_sheet"]) and len(os.listdir(e["orbit_frames"])) == 8
        pts, rgb = load_points_ply(e["points_ply"])
        assert pts.shape == (e["points"], 3) and rgb.shape == (e["points"], 3) and torch.isfinite(pts).all()
        assert e["points"] <= int((d > 0).sum()) and (e["points"] > 0) == bool((d > 0).any())
    for a, b in zip(sorted(runs["plain"].outputs), sorted(cfg.outputs)):
        assert os.path.basename(a) == os.path.basename(b)
        for suffix in (".pt", "_gs.pt"):
            pa, pb = torch.load(a.replace(".pt", suffix)), torch.load(b.replace(".pt", suffix))
            assert torch.equal(pa["latent"], pb["latent"])
