"""ms per iteration of the Gaussian fit (videomv_amd/gs_fit.py), split by stage: forward + state (preprocess, the one host read of the
instance total, bin / sort / blend with the saved state), loss, backward (blend backward + preprocess backward + view sum, one entry
point), Adam — and the blend backward alone from a kernel-free reading: the backward's stage minus a run of the preprocess backward +
view sum (no instance walk).  65 536 random Gaussians in the LGM's unit cube, 24 orbit views at distance 2, at 256^2 and 512^2.
Prints one JSON line per size.   python tools/gs_fit_bench.py [--iters 20] [--sizes 256,512] [--gaussians 65536] [--loss mse|l1_dssim]
--loss-only: instead, on the same images (the start scene's renders against the targets), the L1 + D-SSIM entry point
(vmv_gs_ssim_loss, forward + backward, and forward only) against the torch-eager composition of the same loss (five grouped conv2d +
autograd): medians over --iters calls, one JSON line per size.  --log FILE appends every JSON line to FILE."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def orbit(views, dist=2.0, elevation=15.0):
    from videomv_amd.gs import GaussianRenderer
    P = GaussianRenderer(output_size=16).proj_matrix
    cv, cvp = [], []
    for i in range(views):
        az, el = math.radians(360.0 * i / views), math.radians(elevation)
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


def scene(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 1.2
    op = torch.sigmoid(torch.randn(n, 1, generator=g))
    sc = 0.1 * torch.nn.functional.softplus(torch.randn(n, 3, generator=g) - 3.0)          # LGM activation of small logits
    rot = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    rgb = torch.rand(n, 3, generator=g)
    return torch.cat([pos, op, sc, rot, rgb], dim=1)


def eager_l1_dssim(img, tgt, lam, w2d):
    """the loss a user would otherwise write: torch eager, grouped conv2d, autograd -> (objective, dL/dimage)"""
    P = img.shape[1]
    x = img.detach().requires_grad_(True)
    conv = lambda t: torch.nn.functional.conv2d(t, w2d, padding=5, groups=P)
    mu1, mu2 = conv(x), conv(tgt)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(tgt * tgt) - mu2 * mu2, conv(x * tgt) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    obj = (1 - lam) * (x - tgt).abs().mean() + lam * (1 - m.mean())
    obj.backward()
    return obj.detach(), x.grad


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def loss_only(args, f, size, emit):
    """vmv_gs_ssim_loss against torch eager on the fitter's current renders and targets"""
    from videomv_amd import _lib as L
    from videomv_amd.gs_fit import ssim_loss_params, ssim_workspace
    from videomv_amd.ops import _stream_ptr
    f._forward()
    img, tgt = f.image.reshape(-1, size, size).clone(), f.targets.reshape(-1, size, size).clone()
    P, lam = img.shape[0], args.lambda_dssim
    ws, out, dl = ssim_workspace(P, size, size, img.device), torch.zeros(3, device=img.device), torch.empty_like(img)
    lib = L.load()
    both, fwd = ssim_loss_params(img, tgt, lam, dl, out, ws), ssim_loss_params(img, tgt, lam, None, out, ws)
    hip = median_ms(lambda: L.check(lib.vmv_gs_ssim_loss(C.byref(both), _stream_ptr()), "gs_ssim_loss"), args.iters, args.warmup)
    hip_fwd = median_ms(lambda: L.check(lib.vmv_gs_ssim_loss(C.byref(fwd), _stream_ptr()), "gs_ssim_loss"), args.iters, args.warmup)
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 4.5)
    g = (g / g.sum()).float()
    w2d = torch.outer(g, g).view(1, 1, 11, 11).repeat(P, 1, 1, 1).to(img.device)
    res = {}
    eager = median_ms(lambda: res.update(r=eager_l1_dssim(img.unsqueeze(0), tgt.unsqueeze(0), lam, w2d)), args.iters, args.warmup)
    L.check(lib.vmv_gs_ssim_loss(C.byref(both), _stream_ptr()), "gs_ssim_loss")
    torch.cuda.synchronize()
    obj, grad = res["r"]
    r3 = lambda t: [round(v, 4) for v in t]
    emit(dict(leg="loss_only", planes=P, size=size, lambda_dssim=lam, hip_ms=r3(hip), hip_forward_only_ms=r3(hip_fwd), eager_ms=r3(eager),
              ms_are="median, min, max", eager_over_hip=round(eager[0] / hip[0], 2), objective_hip=float(out[0]), objective_eager=float(obj),
              grad_rel_l2_vs_eager=float((dl - grad[0]).norm() / grad.norm())))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--gaussians", type=int, default=65536)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--loss", choices=("mse", "l1_dssim"), default="mse")
    ap.add_argument("--lambda-dssim", type=float, default=0.2)
    ap.add_argument("--loss-only", action="store_true")
    ap.add_argument("--log", default=None)
    args = ap.parse_args(argv)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as fh:
                fh.write(line + "\n")
    from videomv_amd import _lib as L
    from videomv_amd.gs import GaussianRenderer
    from videomv_amd.gs_fit import GaussianFitter
    from videomv_amd.ops import _stream_ptr
    cv, cvp = orbit(args.views)
    gt = scene(args.gaussians, 1).cuda()
    start = scene(args.gaussians, 2).cuda()
    for size in (int(s) for s in args.sizes.split(",")):
        tg = GaussianRenderer(size).render(gt.unsqueeze(0), cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda(), None,
                                           bg_color=torch.tensor([0.5, 0.5, 0.5]))["image"][0]
        f = GaussianFitter(start, cv.cuda(), cvp.cuda(), tg, bg=(0.5, 0.5, 0.5), loss=args.loss, lambda_dssim=args.lambda_dssim)
        if args.loss_only:
            loss_only(args, f, size, emit)
            continue
        for _ in range(args.warmup):
            f.step()
        torch.cuda.synchronize()
        names = ["forward_state", "loss", "backward", "adam"]
        tot = dict.fromkeys(names, 0.0)
        for _ in range(args.iters):
            ev = []
            f.step(events=ev)
            torch.cuda.synchronize()
            for k, name in enumerate(names):
                tot[name] += ev[k].elapsed_time(ev[k + 1])
        ms = {k: v / args.iters for k, v in tot.items()}
        # the backward's two parts: a backward launch with num_rendered = 0 runs only the preprocess backward + view sum
        q = f._forward()
        f._loss()
        q.pass_.num_rendered = 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            L.check(L.load().vmv_gs_batch_backward(C.byref(q), _stream_ptr()), "gs_batch_backward")
        e1.record()
        torch.cuda.synchronize()
        ms["preprocess_backward_and_view_sum"] = e0.elapsed_time(e1) / args.iters
        ms["blend_backward"] = ms["backward"] - ms["preprocess_backward_and_view_sum"]
        n, VN = f.num_rendered, args.views * args.gaussians
        rec = dict(size=size, gaussians=args.gaussians, views=args.views, instances=n,
                   ms_per_iter=round(sum(tot.values()) / args.iters, 3), ms={k: round(v, 3) for k, v in ms.items()},
                   grad2d_atomic_bytes_max=36 * n, grad_view_bytes=2 * 56 * VN, psnr_now=round(-10 * math.log10(f.evaluate()), 2))
        if args.loss != "mse":
            rec.update(loss=args.loss, lambda_dssim=args.lambda_dssim)
        emit(rec)


if __name__ == "__main__":
    main()
