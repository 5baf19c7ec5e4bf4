#!/usr/bin/env python
"""Rasteriser alone at the LGM-refined step's size (GPU only): 65 536 Gaussians x 24 views at 512 x 512, synthetic Gaussians sized so
that a view has ~0.88 M (tile, Gaussian) instances as bench.py's LGM leg reports.   python tools/experiments/gs_bench.py [reps]
Under `rocprofv3 --kernel-trace --stats` the per-kernel split of the batched pass.
    python tools/experiments/gs_bench.py depth [rounds] [reps]
times `render` and `render_depth` (the blend's depth mode) on that shape with device events: a warm-up of each, then `rounds` rounds
that ALTERNATE the two in one process, `reps` calls per timed interval; per entry the median and the spread (min .. max) of the rounds.
A tree without render_depth (the parent of the change that added it) reports `render` alone, so the production render of two trees can
be compared by running this file on both: the difference counts only beyond the spread of repeated runs of one tree
(profiles/gs_depth_bench.log)."""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from videomv_amd.gs import GaussianRenderer


def scene(n, seed, smax):
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 1.0
    opacity = torch.rand(n, 1, generator=g)
    scale = 0.003 + smax * torch.rand(n, 3, generator=g)
    rot = torch.randn(n, 4, generator=g)
    rot = rot / rot.norm(dim=1, keepdim=True)
    rgb = torch.rand(n, 3, generator=g)
    return torch.cat([pos, opacity, scale, rot, rgb], dim=1)


def cams(views, P, dist=1.5, elevation=15.0):
    cv, cvp = [], []
    for i in range(views):
        az, el = math.radians(360.0 * i / views + 10.0), math.radians(elevation)
        pos = dist * torch.tensor([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
        fwd = -pos / pos.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 1.0, 0.0])); right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        c2w = torch.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, pos
        view = torch.inverse(c2w).transpose(0, 1)
        cv.append(view); cvp.append(view @ P)
    return torch.stack(cv), torch.stack(cvp)


def depth_leg(r, g, cv, cvp, rounds, reps):
    entries = [("render", r.render)] + ([("render_depth", r.render_depth)] if hasattr(r, "render_depth") else [])
    ms = {name: [] for name, _ in entries}
    for name, fn in entries:                  # warm-up: buffers sized, kernels loaded
        for _ in range(2):
            fn(g, cv, cvp, None)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in entries:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn(g, cv, cvp, None)
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / reps)
    print(f"depth leg: 24 views x {g.shape[1]} Gaussians x {r.size}^2, instances {sum(r.last_num_rendered)}, {rounds} rounds x {reps} calls, device events")
    for name, _ in entries:
        v = sorted(ms[name])
        print(f"  {name:13s} median {v[len(v) // 2]:.3f} ms  min {v[0]:.3f}  max {v[-1]:.3f}  spread {v[-1] - v[0]:.3f} ms per 24 views")
    if len(entries) == 2:
        a, b = (sorted(ms[n])[rounds // 2] for n in ("render", "render_depth"))
        print(f"  render_depth / render = {b / a:.3f}")
    else:
        print("  (this tree has no render_depth)")


def main():
    depth = len(sys.argv) > 1 and sys.argv[1] == "depth"
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and not depth else 5
    r = GaussianRenderer(output_size=512, fovy=49.1)
    g = scene(65536, 3, float(os.environ.get("GS_SMAX", "0.03"))).cuda().unsqueeze(0)
    cv, cvp = cams(24, r.proj_matrix)
    cv, cvp = cv.unsqueeze(0).cuda(), cvp.unsqueeze(0).cuda()
    if depth:
        return depth_leg(r, g, cv, cvp, int(sys.argv[2]) if len(sys.argv) > 2 else 9, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    for mode in ("1", "0"):
        os.environ["VMV_GS_BATCH"] = mode
        out = r.render(g, cv, cvp, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = r.render(g, cv, cvp, None)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        print(f"VMV_GS_BATCH={mode}: {1e3 * dt:.3f} ms per 24 views, instances {sum(r.last_num_rendered)} ({sum(r.last_num_rendered) // 24} per view), "
              f"image sum {float(out['image'].double().sum()):.6f} alpha sum {float(out['alpha'].double().sum()):.6f}")


if __name__ == "__main__":
    main()
