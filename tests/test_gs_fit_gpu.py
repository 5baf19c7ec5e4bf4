"""Fitting Gaussians to a view set on the GPU (csrc/raster_bwd.hip through videomv_amd.gs_fit): the forward with saved state, the
backward against fp64 autograd of the oracle's preprocess plus a differentiable blend with the kernels' rules, central differences
through the HIP forward itself, the loss and Adam kernels against torch, convergence, and the t2v entrance's 3-D export."""
import ctypes as C
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FOVY = 39.6
TAN = math.tan(0.5 * math.radians(FOVY))
GROUPS = dict(position=slice(0, 3), opacity=slice(3, 4), scale=slice(4, 7), rotation=slice(7, 11), colour=slice(11, 14))


def _cams(views, dist=1.6, elevation=15.0, az0=10.0):
    """Orbit cameras looking at the origin, in the rasteriser's convention (tests/test_gs_gpu.py::_cams)."""
    from videomv_amd.gs import GaussianRenderer
    P = GaussianRenderer(output_size=16).proj_matrix
    cv, cvp = [], []
    for i in range(views):
        az, el = math.radians(360.0 * i / views + az0), math.radians(elevation)
        pos = dist * torch.tensor([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
        fwd = -pos / pos.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 1.0, 0.0]))
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        c2w = torch.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, pos
        view = torch.inverse(c2w).transpose(0, 1)
        cv.append(view)
        cvp.append(view @ P)
    return torch.stack(cv), torch.stack(cvp)


def _scene(n, seed, spread=0.5, scale=(0.02, 0.08), opacity=(0.2, 0.8)):
    """Opacities below the 0.99 cap and colours inside (0, 1) with a 0.5 background: the image never clamps."""
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 2 * spread
    op = opacity[0] + (opacity[1] - opacity[0]) * torch.rand(n, 1, generator=g)
    sc = scale[0] + (scale[1] - scale[0]) * torch.rand(n, 3, generator=g)
    rot = torch.randn(n, 4, generator=g)
    rot = rot / rot.norm(dim=1, keepdim=True) * (0.8 + 0.4 * torch.rand(n, 1, generator=g))      # not unit: used as given
    rgb = 0.1 + 0.8 * torch.rand(n, 3, generator=g)
    return torch.cat([pos, op, sc, rot, rgb], dim=1)


def _blend_ref(g, view, view_proj, size, bg):
    """Differentiable fp64 forward of one view: oracle.gs_ref.preprocess (no no_grad) + the kernels' blend rules, vectorised over
    pixels — decisions (skip power > 0, alpha < 1/255, stop before T (1 - alpha) < 1e-4, tile rectangle) taken without gradient,
    alpha = min(0.99, o e^power), output clamp(0, 1), background blended with the final T."""
    from oracle.gs_ref import preprocess
    pp = preprocess(g[:, 0:3], g[:, 4:7], g[:, 7:11], view, view_proj, size, TAN)
    idx = torch.nonzero(pp["valid"]).flatten()
    order = idx[torch.argsort(pp["depth"][idx].detach(), stable=True)]
    ys, xs = torch.meshgrid(torch.arange(size, dtype=g.dtype), torch.arange(size, dtype=g.dtype), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    tx, ty = (xs // 16).long(), (ys // 16).long()
    rect = pp["rect"][order]
    inrect = (rect[:, 0:1] <= tx) & (tx < rect[:, 2:3]) & (rect[:, 1:2] <= ty) & (ty < rect[:, 3:4])      # [K, P]
    xy, con = pp["xy"][order], pp["conic"][order]
    dx, dy = xy[:, 0:1] - xs, xy[:, 1:2] - ys
    power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
    alpha = torch.clamp(g[order, 3:4] * torch.exp(power), max=0.99)
    with torch.no_grad():
        hit = inrect & (power <= 0) & (alpha >= 1.0 / 255.0)
        a = torch.where(hit, alpha, torch.zeros_like(alpha))
        T_incl = torch.cumprod(1 - a, dim=0)
        stop = hit & (T_incl < 1e-4)
        keep = hit & (torch.cumsum(stop.to(torch.int32), dim=0) == 0)
    a = torch.where(keep, alpha, torch.zeros_like(alpha))
    T_excl = torch.cumprod(torch.cat([torch.ones_like(a[:1]), 1 - a[:-1]], dim=0), dim=0)
    w = a * T_excl
    Tf = torch.prod(1 - a, dim=0)
    col = w.transpose(0, 1) @ g[order, 11:14] + Tf.unsqueeze(1) * bg.view(1, 3)
    return col.clamp(0, 1).transpose(0, 1).reshape(3, size, size), bool(stop.any())


def _hip_grad(gauss, cv, cvp, wts, size, bg):
    """HIP forward with state + backward for dL/dimage = wts.  -> (grad [B, N, 14], images [B*V, 3, S, S], fitter)."""
    from videomv_amd.gs_fit import GaussianFitter
    B, V = cv.shape[:2]
    f = GaussianFitter(gauss.cuda(), cv.cuda(), cvp.cuda(), torch.zeros(B, V, 3, size, size).cuda(), bg=bg, fovy=FOVY)
    f.gs.copy_(gauss.reshape(-1, 14).cuda())                   # the Gaussians exactly as given (raw quaternions)
    q = f._forward()
    f.dL.copy_(wts.reshape(f.dL.shape).cuda())
    f._backward(q)
    torch.cuda.synchronize()
    return f.grad.reshape(B, -1, 14).cpu().double(), f.image.cpu(), f


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_forward_with_state_is_the_production_render():
    from videomv_amd.gs import GaussianRenderer
    size, bg = 64, (0.3, 0.5, 0.7)
    g = torch.stack([_scene(300, 1), _scene(300, 2, opacity=(0.5, 0.95))])
    cv, cvp = _cams(3)
    cv, cvp = torch.stack([cv, cv.flip(0)]), torch.stack([cvp, cvp.flip(0)])
    ref = GaussianRenderer(size, FOVY).render(g.cuda(), cv.cuda(), cvp.cuda(), None, bg_color=torch.tensor(bg))
    _, img, f = _hip_grad(g, cv, cvp, torch.zeros(6, 3, size, size), size, bg)
    assert torch.equal(img.reshape(ref["image"].shape), ref["image"].cpu())
    assert torch.equal(f.alpha.reshape(ref["alpha"].shape).cpu(), ref["alpha"].cpu())
    T = f.final_T.cpu()
    assert float((T - (1 - f.alpha[:, 0].cpu())).abs().max()) < 2e-5
    assert int(f.n_contrib.max()) > 0 and float(T.min()) < 0.5


# (N, V, S, B, seed, kind): kinds — plain; "stop": dense, opaque cluster (early stop in many pixels); "chunks": > 256 instances in
# a tile (N = 320: a tile holds a Gaussian once per view, so more than one 256-entry LDS chunk needs N > 256), faint so that no pixel
# stops early; "edge": Gaussians beside the frustum, where t.xy / t.z is clamped to +-1.3 tan(fov / 2).  The "chunks" cases at S = 16 are
# ONE tile that holds every Gaussian (checked on the CPU with oracle.gs_ref.preprocess for these seeds: all N valid, rectangle
# [0, 0, 1, 1], the deepest one above the 1/255 cut in > 60 pixels): N = 255 / 256 / 257 make the last chunk an odd tail, exactly full,
# and a lone entry — the boundary of the staging the forward and the backward share, where the forward pads j >= hi and the backward
# pads slots >= n derived from the tile's largest n_contrib.
CASES = [(16, 1, 32, 1, 3, "plain"), (96, 2, 48, 2, 4, "plain"), (256, 4, 64, 1, 5, "plain"), (200, 2, 32, 1, 6, "stop"),
         (320, 1, 32, 1, 7, "chunks"), (64, 2, 48, 1, 8, "edge"),
         (255, 1, 16, 1, 9, "chunks"), (256, 1, 16, 1, 10, "chunks"), (257, 1, 16, 1, 11, "chunks")]


@pytest.mark.parametrize("N,V,S,B,seed,kind", CASES)
def test_backward_matches_fp64_autograd(N, V, S, B, seed, kind):
    """Per-group rel-L2 of the HIP gradient against fp64 autograd <= 1e-3 (the issue's bound; the fp32 T recovery by division and
    the per-tile sums give a spread of a few 1e-5 to a few 1e-4 here)."""
    bg = (0.5, 0.5, 0.5)
    scenes = []
    for b in range(B):
        if kind == "stop":
            s = _scene(N, seed + b, spread=0.15, scale=(0.05, 0.12), opacity=(0.6, 0.95))
        elif kind == "chunks":
            s = _scene(N, seed + b, spread=0.05, scale=(0.15, 0.3), opacity=(0.01, 0.03))
        else:
            s = _scene(N, seed + b)
        if kind == "edge":
            # half of them beside the frustum of view 0 (|x / z| ~ 1.35 - 1.6 tan), wide enough to reach into the image
            cv0, _ = _cams(V)
            c2w = torch.inverse(cv0[0].transpose(0, 1))
            gen = torch.Generator().manual_seed(seed + 100)
            k = N // 2
            z = 1.2 + 0.6 * torch.rand(k, generator=gen)
            xr = (1.35 + 0.25 * torch.rand(k, generator=gen)) * TAN * torch.sign(torch.rand(k, generator=gen) - 0.5)
            yr = (torch.rand(k, generator=gen) - 0.5) * TAN
            pc = torch.stack([xr * z, yr * z, z, torch.ones(k)], dim=1)
            s[:k, 0:3] = (pc @ c2w.transpose(0, 1))[:, :3]
            s[:k, 4:7] = 0.15 + 0.1 * torch.rand(k, 3, generator=gen)
        scenes.append(s)
    g = torch.stack(scenes)
    cv, cvp = _cams(V)
    cv, cvp = cv.unsqueeze(0).expand(B, -1, -1, -1).contiguous(), cvp.unsqueeze(0).expand(B, -1, -1, -1).contiguous()
    wts = torch.randn(B * V, 3, S, S, generator=torch.Generator().manual_seed(seed))
    hip, _, f = _hip_grad(g, cv, cvp, wts, S, bg)
    if kind == "chunks" and N > 256:
        assert int(f.n_contrib.max()) > 256
    if kind == "chunks" and S == 16:
        assert f.num_rendered == N
    ref = torch.zeros_like(hip)
    stopped = False
    for b in range(B):
        gd = g[b].double().clone().requires_grad_(True)
        loss = 0
        for v in range(V):
            img, st = _blend_ref(gd, cv[b, v].double(), cvp[b, v].double(), S, torch.tensor(bg, dtype=torch.float64))
            stopped |= st
            loss = loss + (img * wts[b * V + v].double()).sum()
        loss.backward()
        ref[b] = gd.grad
    if kind == "stop":
        assert stopped
    errs = {k: _rel(hip[..., sl], ref[..., sl]) for k, sl in GROUPS.items()}
    assert all(e <= 1e-3 for e in errs.values()), errs


def test_backward_matches_central_differences_of_the_hip_forward():
    """A second witness that does not use the test's blend: central differences of sum(w * image) through the HIP forward, one
    Gaussian, every one of its 14 parameters (step 1e-3 on the fp32 forward: differences of ~1e-6 relative in a sum of ~1e3 terms).
    The weights vanish where the unperturbed alpha is below 0.02: the 1/255 alpha cut is a step of the forward that the gradient
    (by the rules, like autograd's) does not see, and pixels crossing it under a perturbation would otherwise add O(1) to the
    differences whatever the step."""
    from videomv_amd.gs import GaussianRenderer
    S, bg = 32, (0.5, 0.5, 0.5)
    g = torch.tensor([[0.02, -0.03, 0.05, 0.6, 0.12, 0.08, 0.1, 0.9, 0.2, -0.3, 0.1, 0.8, 0.3, 0.6]])
    cv, cvp = _cams(1)
    cv, cvp = cv.unsqueeze(0), cvp.unsqueeze(0)
    r = GaussianRenderer(S, FOVY)
    alpha = r.render(g.unsqueeze(0).cuda(), cv.cuda(), cvp.cuda(), None, bg_color=torch.tensor(bg))["alpha"][0, 0].cpu()
    wts = torch.randn(1, 3, S, S, generator=torch.Generator().manual_seed(0)) * (alpha > 0.02)
    assert float((alpha > 0.02).float().mean()) > 0.1
    hip, _, _ = _hip_grad(g.unsqueeze(0), cv, cvp, wts, S, bg)
    L = lambda x: float((r.render(x.unsqueeze(0).cuda(), cv.cuda(), cvp.cuda(), None, bg_color=torch.tensor(bg))["image"][0, 0].cpu().double()
                         * wts[0].double()).sum())
    h = 1e-3
    fd = torch.zeros(14, dtype=torch.float64)
    for k in range(14):
        gp, gm = g.clone(), g.clone()
        gp[0, k] += h
        gm[0, k] -= h
        fd[k] = (L(gp) - L(gm)) / (2 * h)
    assert _rel(hip[0, 0], fd) < 1e-2, (hip[0, 0], fd)


def test_loss_and_adam_kernels_match_torch():
    from videomv_amd import _lib as L
    from videomv_amd.ops import _stream_ptr
    gen = torch.Generator().manual_seed(1)
    img, tgt = torch.rand(3, 3, 37, 41, generator=gen).cuda(), torch.rand(3, 3, 37, 41, generator=gen).cuda()
    dl, loss, ws = torch.empty_like(img), torch.zeros(1).cuda(), torch.empty(1024).cuda()
    L.check(L.load().vmv_gs_image_loss(img.data_ptr(), tgt.data_ptr(), img.numel(), dl.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream_ptr()))
    x = img.clone().requires_grad_(True)
    ref = torch.nn.functional.mse_loss(x, tgt)
    ref.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ref)) <= 1e-6 * float(ref) and _rel(dl.cpu().double(), x.grad.cpu().double()) < 1e-6
    # Adam on the raw parameters through the activation chain, 5 groups, 6 steps
    from videomv_amd.gs_fit import gaussians_to_raw
    n = 1000
    raw = gaussians_to_raw(_scene(n, 9)).cuda()
    lrs = [1e-3, 5e-2, 5e-3, 1e-3, 2.5e-3]
    leaves = [raw[:, sl].clone().requires_grad_(True) for sl in GROUPS.values()]
    opt = torch.optim.Adam([dict(params=[t], lr=lr) for t, lr in zip(leaves, lrs)], betas=(0.9, 0.999), eps=1e-15)
    params, m, v = raw.clone(), torch.zeros_like(raw), torch.zeros_like(raw)
    out, grad = torch.empty_like(raw), torch.empty_like(raw)
    for t in range(1, 7):
        G = torch.randn(n, 14, generator=gen).cuda()
        opt.zero_grad()
        p, o, s, q, f = leaves
        act = torch.cat([p, torch.sigmoid(o), torch.exp(s), torch.nn.functional.normalize(q, dim=-1), 0.28209479177387814 * f + 0.5], dim=1)
        (act * G).sum().backward()
        opt.step()
        grad.copy_(G)
        a = L.GsAdamParams()
        a.params, a.m, a.v, a.grad, a.gaussians, a.n, a.step = params.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), out.data_ptr(), n, t
        for i, lr in enumerate(lrs):
            a.lr[i] = lr
        a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-15
        L.check(L.load().vmv_gs_adam_step(C.byref(a), _stream_ptr()))
        torch.cuda.synchronize()
        for (k, sl), leaf in zip(GROUPS.items(), leaves):
            assert _rel(params[:, sl].double(), leaf.detach().double()) <= 1e-6, (t, k)
    with torch.no_grad():
        p, o, s, q, f = leaves
        act = torch.cat([p, torch.sigmoid(o), torch.exp(s), torch.nn.functional.normalize(q, dim=-1), 0.28209479177387814 * f + 0.5], dim=1)
    assert _rel(out.double(), act.double()) <= 1e-6


def _orbit_scene(seed=21, n=400, views=24, size=64):
    from videomv_amd.gs import GaussianRenderer
    gt = _scene(n, seed, spread=0.35, scale=(0.03, 0.07), opacity=(0.3, 0.9))
    gt[:, 7:11] = gt[:, 7:11] / gt[:, 7:11].norm(dim=1, keepdim=True)          # the fitter's activation normalises
    cv, cvp = _cams(views, dist=2.0)
    tg = GaussianRenderer(size, FOVY).render(gt.unsqueeze(0).cuda(), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None,
                                             bg_color=torch.tensor([0.5, 0.5, 0.5]))["image"][0]
    return gt, cv, cvp, tg


def test_fit_converges_and_stays_at_the_ground_truth():
    from videomv_amd.gs_fit import GaussianFitter
    gt, cv, cvp, tg = _orbit_scene()
    gen = torch.Generator().manual_seed(5)
    pert = gt.clone()
    pert[:, 0:3] += 0.01 * torch.randn(gt.shape[0], 3, generator=gen)
    pert[:, 3] = (pert[:, 3] + 0.2 * torch.randn(gt.shape[0], generator=gen)).clamp(0.05, 0.95)
    pert[:, 4:7] *= torch.exp(0.2 * torch.randn(gt.shape[0], 3, generator=gen))
    pert[:, 11:14] = (pert[:, 11:14] + 0.15 * torch.randn(gt.shape[0], 3, generator=gen)).clamp(0.02, 0.98)
    f = GaussianFitter(pert.cuda(), cv.cuda(), cvp.cuda(), tg, bg=(0.5, 0.5, 0.5), fovy=FOVY)
    st = f.fit(100)
    print("perturbed:", st)
    # calibrated once on an MI355X: 100 iterations took this scene from 26.1 to 37.2 dB (+11.1); the 8 dB margin leaves room for
    # the order-dependent last bits of the float-atomic gradient sums, which steer the trajectory slightly from run to run
    assert st["psnr_after"] > st["psnr_before"] + 8.0 and st["loss_after"] < st["loss_before"]
    f0 = GaussianFitter(gt.cuda(), cv.cuda(), cvp.cuda(), tg, bg=(0.5, 0.5, 0.5), fovy=FOVY)
    st0 = f0.fit(20)
    print("from the ground truth:", st0)
    # at the optimum Adam's normalised steps still move every parameter by about its learning rate (the gradients are rounding
    # noise): calibrated once on an MI355X, 20 of them left the renders at 51 dB (from 119 dB, the raw -> activated round trip)
    assert st0["psnr_before"] > 60 and st0["psnr_after"] > 45
    assert f0.gaussians().shape == (gt.shape[0], 14)


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


def test_t2v_entrance_exports_fitted_gaussians(tmp_path):
    """Two prompts, save_gaussians with a 20-iteration fit and 8 orbit views: ply, sheet and frames per prompt, the fit lowers the
    loss, and both prompts' latents are the bits of the run without the keys (the export draws nothing from the torch RNG)."""
    from videomv_amd.registry import INFER_ENGINE
    from videomv_amd.gs import GaussianRenderer
    import videomv_amd.entrance  # noqa: F401
    runs = {}
    for name, extra in (("plain", []), ("export", ["save_gaussians", "True", "gs_fit_iters", "20", "gs_orbit_views", "8"])):
        cu = _entrance_cfg(tmp_path / name, extra)
        runs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    cfg = runs["export"]
    assert len(cfg.gs_exports) == 2
    for e in cfg.gs_exports:
        g = GaussianRenderer.load_ply(e["ply"])
        assert 0 < g.shape[0] <= 64 * 64 * 4 and torch.isfinite(g).all()
        assert os.path.exists(e["orbit_sheet"]) and len(os.listdir(e["orbit_frames"])) == 8
        assert e["loss_after"] < e["loss_before"] and e["ms_per_iter"] > 0
    for a, b in zip(sorted(runs["plain"].outputs), sorted(cfg.outputs)):
        assert os.path.basename(a) == os.path.basename(b)
        for suffix in (".pt", "_gs.pt"):
            pa, pb = torch.load(a.replace(".pt", suffix)), torch.load(b.replace(".pt", suffix))
            assert torch.equal(pa["latent"], pb["latent"])
