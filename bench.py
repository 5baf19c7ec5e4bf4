#!/usr/bin/env python
"""bench.py — denoise-steps/s of the HIP hot path on MI355X (BASELINE.json metric).

One "step" = one DDIM denoising step of the t2v sampler on one 24-view sample:
    [cond | uncond] UNetSD_T2VBase pass (full-size: dim 320, 1.413 B params, 16-bit storage (VMV_DTYPE: fp16 default | bf16) / fp32 accumulate)
    + classifier-free guidance + x0 + DDIM update                      (diffusion_ddim.py:149-160,192-195,233-243)
Workload (BASELINE.json configs[1]): t2v_infer.yaml shape, 24 views, 320x512 px = latent [1,4,24,40,64], 77 text
tokens, guide 9.0, linear_sd schedule, 50-step timestep list (981..1) cycled over the timed steps.
Synthetic data: seeded randn latents / text features, the entrance's real orbit cameras (get_camera 24 x elevation 15,
distance 2.0 + the row flips: videomv_amd/camera.py); random-init
weights of the reference architecture with the zero-inits re-randomised (no checkpoint ships).

N > 1 (launched by torch.distributed.run, one rank per GPU, RCCL): every rank denoises its OWN sample — replicas,
the reference's only parallelism (inference_text2video_entrance.py:79,152-156) — so scaling is weak and there is no
data-path collective; `value` = (N * K steps) / max-over-ranks time.  The same run then times the frame-parallel mode
(BASELINE configs[2]: ONE sample, 24/N views per GPU, all-to-all layout switches + gathered GroupNorm sums over RCCL,
DESIGN.md §8) and reports it as the extra object `frame_parallel` (strong scaling of one sample's latency); a watchdog
bounds that leg so that a collective problem can never cost the headline line.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the --steps steps and prints the headline; everything
else is measured only with --full: the extra objects `roofline` (dominant kernel = the MFMA implicit-GEMM family, timed per
launch with events on the launch stream in a separate pass), `reference_shape`, `prompt_batch`, the N > 1 frame-parallel leg,
the complete samples (24-view + VAE, CLIP towers, LGM-refined, I2VGen), `simulated_rank`, `other_dtype` and `cpu_baseline`
(the oracle's fp32 UNet forward on the host cores, bounded sample, FLOP-scaled to the metric's unit); the --no-* options
trim a --full run.  --dump-outputs DIR writes the latent the last timed step left (rank 0) as DIR/latent.npy (float32).
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FULL = dict(in_dim=4, dim=320, context_dim=1024, out_dim=4, dim_mult=[1, 2, 4, 4], num_heads=8, head_dim=64,
            num_res_blocks=2, attn_scales=[1.0, 0.5, 0.25])
PEAK_MFMA16_TFLOPS = 2500.0      # dense MFMA fp16 / bf16 (same rate), MI355X_MICROARCH.md
STEP_TFLOP = {(32, 32): 2 * 7.336, (40, 64): 2 * 18.885}     # 2 UNet forwards per step


def randomize_(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for name, p in model.named_parameters():
        if p.dim() == 1:
            if name.endswith(".bias"):
                p.normal_(0.0, 0.05, generator=g)
            else:
                p.normal_(1.0, 0.1, generator=g)
        else:
            fan_in = p[0].numel()
            p.normal_(0.0, 1.0 / math.sqrt(fan_in), generator=g)


# cpu_baseline: the oracle's UNet forward at the bench shape itself when the host can finish it inside the budget, else
# the reference's own 32x32 shape, else a small latent — never scaled by pixel count; the JSON says which one ran
CPU_BUDGET_S = 150.0
_OPEN_COMMS = []       # FrameComm / CfgFrameComm objects of this process: closed before dist.destroy_process_group()


def _cpu_baseline_worker(frames, threads, H, W, budget):
    """Runs in a child process: oracle UNet forwards (fp32 torch-CPU eager, full-size architecture; the same math as the
    reference's CPU/eager path — oracle/unet_ref.py, pinned to reference goldens).  A small forward first (page-in, thread
    pool, and a time estimate), then ONE forward at the largest of {HxW, 32x32} predicted to fit the budget."""
    from oracle.unet_ref import UNetCfg, unet_forward
    from oracle.weights import unet_param_shapes
    torch.set_num_threads(threads)
    ocfg = UNetCfg(**FULL)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in unet_param_shapes(ocfg).items():
        if len(shp) == 1:
            sd[k] = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
        else:
            sd[k] = torch.empty(shp).normal_(0.0, 0.02, generator=g)
    y = torch.randn(1, 77, 1024, generator=g)
    cam = torch.randn(1, frames, 16, generator=g)
    t1 = torch.tensor([501])

    def run(h, w):
        x = torch.randn(1, 4, frames, h, w, generator=g)
        t0 = time.time()
        unet_forward(sd, ocfg, x, t1, y, cam)
        dt = time.time() - t0
        print("CPU_FWD", h, w, dt, flush=True)
        return dt

    run(8, 8)                       # warm-up
    t8 = run(8, 8)
    for h, w in ((H, W), (32, 32)):
        if h * w <= 64 or h * w > H * W:
            continue
        # conv / linear work scales with pixels, spatial attention faster; large shapes use the cores better: x0.6 .. x1.5
        if t8 * (h * w / 64.0) * 0.6 < budget:
            run(h, w)
            break


def physical_cores(logical):
    """Physical cores this process may use ("host cores, count stated"): psutil's physical count, capped by the affinity mask."""
    try:
        import psutil
        ph = psutil.cpu_count(logical=False) or logical
    except Exception:
        ph = logical
    return max(1, min(ph, logical))


def cpu_baseline(frames, cores, shape, threads=None, budget=None):
    """Oracle (`port`) timed on the host in a child process with a hard time budget, on `threads` threads (default min(host cores,
    64): torch-CPU eager stops scaling beyond that on these shapes).  Returns (seconds per forward, threads, (h, w))."""
    import subprocess
    threads = max(1, min(cores, threads or 64))
    budget = float(budget or CPU_BUDGET_S)
    code = f"import bench; bench._cpu_baseline_worker({frames}, {threads}, {shape[0]}, {shape[1]}, {budget})"
    out = ""
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1.5 * budget + 90)
        out = r.stdout
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
    best = None
    for line in out.splitlines():
        if line.startswith("CPU_FWD"):
            _, h, w, dt = line.split()
            if best is None or int(h) * int(w) >= best[2][0] * best[2][1]:
                best = (float(dt), threads, (int(h), int(w)))
    return best if best else (None, threads, None)


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs: each tensor as d/<name>.npy in float32 (what the timed path left, so that two builds can be compared output for
    output).  Past DUMP_CAP_BYTES in all, each tensor is replaced by a fixed seeded sample of its flattened elements (<name>_sample.npy)."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    total = sum(4 * t.numel() for t in arrays.values())
    for name, t in arrays.items():
        a = t.detach().float().cpu()
        if total > DUMP_CAP_BYTES:
            keep = max(1, a.numel() * DUMP_CAP_BYTES // total)      # (this tensor's share of the cap, in 4-byte elements)
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values
            a, name = a.reshape(-1)[idx], name + "_sample"
        np.save(os.path.join(d, name + ".npy"), a.numpy().astype(np.float32))


def kernel_sources_sha16():
    """sha256 (first 16 hex digits) over the HIP sources the library is built from — what a committed counter measurement is tied to:
    `roofline.traffic` comes from profiles/*_gemm_traffic.json (PMC passes cannot run inside the timed process) and is marked stale
    when the kernels have changed since (no .git on the GPU box: the tree's own bytes are the reference)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "videomv_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(d, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def _device_count():
    """GPUs this process may use (VMV_BENCH_FAKE_DEVICES: the CPU test of the launcher pretends to have some)."""
    fake = os.environ.get("VMV_BENCH_FAKE_DEVICES")
    return int(fake) if fake else torch.cuda.device_count()


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(n, argv):
    """``python bench.py --gpus N`` with no launcher around it (WORLD_SIZE unset): start the N ranks HERE, one process per GPU, the way
    the reference's entrance starts its workers (mp.spawn over the visible devices, inference_text2video_entrance.py:55-61) and with the
    environment torch.distributed.run would have set (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR = 127.0.0.1 / MASTER_PORT).  Rank 0
    prints the one JSON line on the inherited stdout.  A rank that dies takes the others down (exact PIDs, never by pattern); the exit
    code is the first non-zero one."""
    import subprocess
    have = _device_count()
    if have < n and os.environ.get("VMV_BENCH_SHARE_GPU") != "1":
        raise SystemExit(f"--gpus {n} but only {have} GPU(s) are visible to this process")
    port = int(os.environ.get("MASTER_PORT") or _free_port())
    script = os.path.abspath(__file__)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VMV_BENCH_LAUNCHER="self-spawned")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # (dmabuf IPC: RCCL between processes needs it on this pool)
        procs.append(subprocess.Popen([sys.executable, script] + list(argv), env=env, cwd=os.getcwd(),
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        alive = list(procs)
        while alive:
            for p_ in list(alive):
                code = p_.poll()
                if code is None:
                    continue
                alive.remove(p_)
                if code != 0 and rc == 0:
                    rc = code
                    for q in alive:                       # one rank failed: the others would wait in a collective for ever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
    return rc


def run_fp_children(args, rank, world, local_launcher, port, dry_run=False):
    """The frame-parallel leg (BASELINE configs[2]) of an N > 1 run in CHILD processes, one per rank, with a process group of their own.

    Why: that leg is the one part of the bench no round could run on real peers (in-plan RCCL all-to-all / all-gather at world > 1 has
    only met gloo, a simulated rank and world-1 RCCL), and a GPU fault or a native abort there would take the rank — and under
    torch.distributed.run every rank — down BEFORE the replica line (`value`, the scaling curve's point) is printed.  In children the
    worst case is `frame_parallel: {error}` beside an intact headline.  Each child is this script again with --fp-inprocess and the
    same RANK / LOCAL_RANK / WORLD_SIZE, a fresh MASTER_PORT (`port`, agreed by the parents) and without the TORCHELASTIC_* variables
    (the agent's store serves the parents' port only).  Returns the dict for the line's `frame_parallel` (rank 0) or None."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
               VMV_BENCH_LAUNCHER=f"frame-parallel child of {local_launcher}")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--latent", args.latent, "--frames", str(args.frames), "--full", "--fp-inprocess", "--frame-parallel-budget", str(args.frame_parallel_budget),
           "--no-cpu-baseline", "--no-op-profile", "--no-sample", "--no-lgm", "--no-i2vgen", "--simulate-rank", "0"]
    if dry_run:
        cmd.append("--pg-dry-run")
    limit = 60.0 if dry_run else args.frame_parallel_budget + 150.0      # (the child's own watchdog fires at the budget; + start-up: imports, model build, headline warm-up)
    out, err = "", None
    p_ = subprocess.Popen(cmd, env=env, cwd=os.getcwd(), stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, text=True)
    try:
        out, _ = p_.communicate(timeout=limit)
        if p_.returncode != 0:
            err = f"child exited with code {p_.returncode}"
    except subprocess.TimeoutExpired:
        p_.kill()                                 # (exact PID)
        try:
            out, _ = p_.communicate(timeout=20)
        except Exception:
            out = ""
        err = f"child did not finish inside {limit:.0f} s"
    if rank != 0:
        return None
    line = next((l for l in (out or "").splitlines()[::-1] if l.startswith("{")), None)
    dj = None
    if line:
        try:
            dj = json.loads(line)
        except Exception:
            dj = None
    if dry_run:
        return dict(dj or {}, **({"error": err} if err else {}))
    fp = (dj or {}).get("frame_parallel")
    if not isinstance(fp, dict):
        fp = dict(error=err or "the child printed no frame_parallel object")
    elif err and "error" not in fp:
        fp["error"] = err
    fp["isolation"] = "child processes with their own process group (a fault in this leg cannot cost the replica line)"
    if dj and "rccl_ranks" in dj:
        fp["child_rccl_ranks"] = dj["rccl_ranks"]
    return fp


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--latent", type=str, default="40x64", help="latent HxW (40x64 = 320x512 px; 32x32 = reference 256 px)")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--full", action="store_true", help="also run every measurement beyond the headline (roofline, reference shape, prompts "
                    "per plan, N > 1 frame-parallel leg, samples, simulated rank, CPU baseline); the --no-* options below trim it")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR", help="after the timed steps, write the latent the last one left "
                    "(rank 0) as DIR/latent.npy, float32 (a fixed seeded sample of it when it exceeds 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-op-profile", action="store_true")
    ap.add_argument("--dump-ops", type=str, default="", help="write the per-launch timing table to this file")
    ap.add_argument("--no-frame-parallel", action="store_true", help="N > 1: skip the frame-parallel (one sample over all GPUs) leg")
    ap.add_argument("--frame-parallel-budget", type=float, default=150.0, help="seconds before the watchdog abandons that leg (a healthy leg "
                    "takes 30-40 s at 8 ranks: seven sub-legs of ~12 steps + their plan builds)")
    ap.add_argument("--fp-inprocess", action="store_true", help="N > 1: run the frame-parallel leg inside the rank processes themselves (what the "
                    "leg's child processes do); default: in one child process per rank, so that a fault there cannot cost the replica line")
    ap.add_argument("--no-prompt-batch", action="store_true", help="skip the two-prompts-per-plan throughput leg")
    ap.add_argument("--no-lgm", action="store_true", help="skip the LGM-refined sample (BASELINE configs[4])")
    ap.add_argument("--no-sample", action="store_true", help="skip the (untimed-region) full 50-step + VAE-decode sample")
    ap.add_argument("--simulate-rank", type=int, default=8, metavar="W", help="N = 1 only: also build rank 0's plan of a W-GPU frame-parallel run "
                    "(BASELINE configs[2]: 24 / W views, HW / W pixels per temporal block) on THIS GPU with the W - 1 peers simulated — every "
                    "collective a local copy of the same bytes — and report its GPU and host ms per step; 0 = skip")
    ap.add_argument("--dump-ops-sim", type=str, default="", help="per-launch timing table of the simulated rank's plan")
    ap.add_argument("--no-i2vgen", action="store_true", help="skip the UNetSD_I2VGen leg (BASELINE configs[3])")
    ap.add_argument("--no-alt-dtype", action="store_true", help="(default since round 3; kept for old command lines)")
    ap.add_argument("--alt-dtype", action="store_true", help="also time the other 16-bit element type's library in a child process "
                    "(bf16 is the range fallback — DESIGN.md §6 — and not part of the headline line)")
    ap.add_argument("--pg-dry-run", action="store_true", help="(launcher test) join the process group, count the ranks, print the line's "
                    "launch fields and exit before any GPU work; VMV_BENCH_PG_BACKEND=gloo lets it run without GPUs")
    args = ap.parse_args(argv)
    H, W = (int(v) for v in args.latent.split("x"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher around us: be the launcher (VERDICT r5 #1 — `python bench.py --gpus 8` used to time ONE GPU and say n_gpus: 1)
        rc = launch_ranks(args.gpus, argv)
        if rc:
            raise SystemExit(rc)
        return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    backend = os.environ.get("VMV_BENCH_PG_BACKEND", "nccl")          # nccl IS RCCL on ROCm; gloo only for the launcher's CPU test
    # VMV_BENCH_SHARE_GPU=1 (with the gloo backend): every rank on device 0, collectives staged through the host (comm.FrameComm) — the
    # whole N > 1 flow (launcher, replica timing, frame-parallel legs) smoke-tested on a ONE-GPU box; never a measurement
    share_gpu = os.environ.get("VMV_BENCH_SHARE_GPU") == "1" and backend == "gloo"
    if share_gpu:
        local = 0
    if backend == "nccl" or share_gpu:
        if _device_count() <= local:
            raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but only {_device_count()} GPU(s) visible")
        torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    cdev = dev if backend == "nccl" else torch.device("cpu")          # where the bench's own small collectives live
    dist, rccl_ranks = None, None
    if world > 1 or os.environ.get("VMV_BENCH_FORCE_PG") == "1":     # (forced at world 1 only to smoke-test the RCCL path)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # the ranks that actually JOINED the communicator, counted by the communicator itself: one all-reduce of a 1 per rank
        one = torch.ones(1, dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(one)
        rccl_ranks = int(one[0])
        if rccl_ranks != world:
            raise SystemExit(f"process group of {world} ranks counted {rccl_ranks}")
    launcher = os.environ.get("VMV_BENCH_LAUNCHER") or ("torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else
                                                        ("none (single process)" if world == 1 else "external"))
    def agreed_port():
        """A free port picked by rank 0 and handed to every rank through the parents' own process group (for the children's group)."""
        pt = torch.tensor([_free_port() if rank == 0 else 0], dtype=torch.int32, device=cdev)
        dist.all_reduce(pt)
        return int(pt[0])

    fp_children = args.full and dist is not None and world > 1 and args.frames % world == 0 and not args.no_frame_parallel and not args.fp_inprocess
    if args.pg_dry_run:
        fp_child = run_fp_children(args, rank, world, launcher, agreed_port(), dry_run=True) if fp_children else None
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "rccl_ranks": rccl_ranks, "pg_backend": backend if dist is not None else None,
                              "launcher": launcher, "steps": args.steps, "warmup": args.warmup, "fp_child": fp_child}), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    from videomv_amd import _lib
    _lib.load()      # the product path fails loudly without the HIP extension
    from videomv_amd.registry import MODEL, DIFFUSION
    import videomv_amd.unet_t2v  # noqa: F401
    import videomv_amd.diffusion_ddim  # noqa: F401
    from videomv_amd import _lib as L
    from videomv_amd.flops import gemm_flops, attn_flops, gemm_bytes

    with torch.device(dev):
        model = MODEL.build(dict(type="UNetSD_T2VBase", y_dim=1024, use_camera_condition=True, use_lgm_refine=False, **FULL))
    randomize_(model, 1234)
    model.eval()
    dif = DIFFUSION.build(dict(type="DiffusionDDIM", schedule="linear_sd",
                               schedule_param=dict(num_timesteps=1000, init_beta=0.00085, last_beta=0.012,
                                                   zero_terminal_snr=False), mean_type="eps", var_type="fixed_small"))
    g = torch.Generator(device=dev).manual_seed(11 + rank)     # t2v_infer.yaml seed (+rank, as the reference)
    noise = torch.randn(1, 4, args.frames, H, W, generator=g, device=dev)
    y = torch.randn(1, 77, 1024, generator=g, device=dev)
    y0 = torch.randn(1, 77, 1024, generator=g, device=dev)
    from videomv_amd.camera import entrance_camera_data
    cam = entrance_camera_data(args.frames, elevation=15, camera_distance=2.0).to(dev)   # the entrance's real orbit cameras (§8d)
    steps = [int(s) for s in dif.ddim_steps(50)]
    stride = 1000 // 50
    xt = noise.clone()

    kw_c, kw_u = dict(y=y, camera_data=cam), dict(y=y0, camera_data=cam)

    def one_step(i):
        dif.ddim_step_hip(xt, steps[i % len(steps)], model, kw_c, kw_u, 9.0, stride)

    for i in range(args.warmup):
        one_step(i)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        one_step(args.warmup + i)
    fence()
    dt = time.perf_counter() - t0
    from videomv_amd.dist import max_over_ranks
    dt = max_over_ranks(dt, cdev)                # the slowest rank defines the job time (no-op at N = 1)
    finite = bool(torch.isfinite(xt).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(latent=xt))
    steps_per_s = world * args.steps / dt
    ms_per_step = 1000.0 * dt / args.steps
    step_tflop = STEP_TFLOP.get((H, W))

    # ---- per-launch timing pass (events on the launch stream = torch's current stream)
    KIND = {L.OP_GEMM: "gemm", L.OP_GN_STATS: "gn_stats", L.OP_GN_APPLY: "gn_apply", L.OP_LAYERNORM: "layernorm",
            L.OP_ATTENTION: "attention", L.OP_GN_FUSED: "gn_fused", L.OP_COPY: "copy", L.OP_FF: "ff_fused", L.OP_GN_TABLE: "gn_table",
            L.OP_COMM: "collective"}

    def op_flops(op, p):
        return gemm_flops(p) if op == L.OP_GEMM else (attn_flops(p) if op == L.OP_ATTENTION else 0.0)

    def profile_plan(eng, reps=3, dump=""):
        """Every recorded launch of `eng`'s plan timed on its own (events on the launch stream, min of `reps`).  Returns
        (per-family dict, per-launch ms list)."""
        rec, labels = eng.S.recorded, eng.S.labels
        n = len(rec)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(n + 1)] for _ in range(reps)]
        for r in range(reps):
            torch.cuda.synchronize()
            ev[r][0].record()
            for i in range(n):
                eng.S.run(i, i + 1)
                ev[r][i + 1].record()
        torch.cuda.synchronize()
        ms = [min(ev[r][i].elapsed_time(ev[r][i + 1]) for r in range(reps)) for i in range(n)]
        fam = {}
        for i, (op, p) in enumerate(rec):
            f = fam.setdefault(KIND[op], dict(ms=0.0, flops=0.0, n=0))
            f["ms"] += ms[i]; f["flops"] += op_flops(op, p); f["n"] += 1
        if dump:
            os.makedirs(os.path.dirname(os.path.abspath(dump)), exist_ok=True)
            with open(dump, "w") as f:
                f.write("idx\tlabel\tms\tGFLOP\tTFLOP/s\ttile\n")
                for i, (op, p) in enumerate(rec):
                    fl = op_flops(op, p)
                    tile = eng.S.lib.vmv_gemm_pick_tile(ctypes.byref(p)) if op == L.OP_GEMM else ""
                    f.write(f"{i}\t{labels[i]}\t{ms[i]:.4f}\t{fl / 1e9:.2f}\t{(fl / (ms[i] * 1e-3) / 1e12) if fl else 0:.1f}\t{tile}\n")
        return fam, ms

    def fam_table(fam):
        tot_ms = sum(f["ms"] for f in fam.values())
        return {k: dict(ms=round(v["ms"], 3), share=round(v["ms"] / tot_ms, 4), launches=v["n"],
                        tflops=round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] else None) for k, v in fam.items()}, tot_ms

    roof = None
    if rank == 0 and args.full and not args.no_op_profile:
        eng = model.engine_for(2, args.frames, H, W, 77, dev, n_t=1, share_prefix=True)     # the plan the timed steps replayed
        rec = eng.S.recorded
        fam, _ = profile_plan(eng, dump=args.dump_ops)
        families, tot_ms = fam_table(fam)
        gm = fam["gemm"]
        ach = gm["flops"] / (gm["ms"] * 1e-3) / 1e12
        # HBM bytes per launch of the same family from the committed PMC passes of this command (tools/gemm_traffic.py;
        # FETCH_SIZE doubled as the microarch guide prescribes for gfx950) — counters cannot be read from inside the run
        traffic, traffic_src, traffic_stale = None, None, None
        tpath = next((q for q in (os.path.join(ROOT, "profiles", f"r{r}_gemm_traffic.json") for r in (6, 5, 4, 3)) if os.path.exists(q)), None)
        if (H, W) == (40, 64) and args.frames == 24 and tpath:
            with open(tpath) as f:
                tj = json.load(f)
            traffic = round(tj["bytes_per_launch"])
            # stale = the kernels were edited after the counters were read (last bundle's number on this run's line)
            traffic_stale = tj.get("sources_sha16") != kernel_sources_sha16()
            traffic_src = (f"profiles/{os.path.basename(tpath)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, separate runs, "
                           f"kernel sources {tj.get('sources_sha16', 'unrecorded')}, dtype {tj.get('dtype', '?')}; per-kernel table: "
                           f"profiles/r6_gemm_traffic_by_kernel.tsv)" + (" — STALE: the kernel sources changed since" if traffic_stale else ""))
        roof = dict(bound="mfma", kernel="16-bit MFMA implicit-GEMM family (gemm_xglds_kernel / gemm_rs_kernel / gemm_glds_kernel / gemm_pglds_kernel / gemm_kernel: "
                    "conv3x3, temporal conv, linear)",
                    achieved=round(ach, 1), peak=PEAK_MFMA16_TFLOPS, unit="TFLOP/s", frac=round(ach / PEAK_MFMA16_TFLOPS, 4),
                    traffic=traffic, traffic_source=traffic_src, traffic_stale=traffic_stale,
                    algorithmic_bytes_per_launch=round(sum(gemm_bytes(p) for op, p in rec if op == L.OP_GEMM) / gm["n"]),
                    launches=gm["n"], avg_launch_us=round(1000.0 * gm["ms"] / gm["n"], 2),
                    flop_per_launch=gm["flops"] / gm["n"], families=families, serial_forward_ms=round(tot_ms, 3))
        if step_tflop:
            roof["whole_step"] = dict(algorithmic_tflop=step_tflop, achieved=round(step_tflop * steps_per_s / world, 1),
                                      frac=round(step_tflop * steps_per_s / world / PEAK_MFMA16_TFLOPS, 4))

    # ---- the reference's OWN shape (256 px = latent 24 x 32 x 32): the same timed loop on that latent, with the
    #      default tile policy + rule and whatever the packaged table adds; `no_table_ms_per_step` is the same with VMV_TUNED=0 semantics
    #      (a fresh engine recorded while the table is hidden), i.e. what an UNTABLED shape gets
    ref_shape = None
    if rank == 0 and world == 1 and (H, W) == (40, 64) and args.full and not args.no_op_profile:
        from videomv_amd import ops as _ops

        def time_shape(h, w, n=10):
            x = torch.randn(1, 4, args.frames, h, w, generator=g, device=dev)
            for i in range(3):
                dif.ddim_step_hip(x, steps[i], model, kw_c, kw_u, 9.0, stride)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                dif.ddim_step_hip(x, steps[(3 + i) % len(steps)], model, kw_c, kw_u, 9.0, stride)
            torch.cuda.synchronize()
            return 1000.0 * (time.perf_counter() - t0) / n, bool(torch.isfinite(x).all())
        try:
            ms32, fin32 = time_shape(32, 32)
            e32 = model.engine_for(2, args.frames, 32, 32, 77, dev, n_t=1, share_prefix=True)
            ref_shape = dict(latent=f"{args.frames}x32x32", ms_per_step=round(ms32, 3), steps_per_s=round(1000.0 / ms32, 3), finite=fin32,
                             whole_step=dict(algorithmic_tflop=STEP_TFLOP[(32, 32)], achieved=round(STEP_TFLOP[(32, 32)] / (ms32 * 1e-3), 1),
                                             frac=round(STEP_TFLOP[(32, 32)] / (ms32 * 1e-3) / PEAK_MFMA16_TFLOPS, 4)),
                             launches_from_table=e32.n_tuned, launches_from_rule=e32.n_ruled)
            # the same shape with the table hidden (rule + built-in policy only) and with neither (built-in policy only): fresh engines
            keep_tab, keep_eng = _ops._TUNED, dict(model._engines) if hasattr(model, "_engines") else None
            for tag, env in (("no_table", {}), ("policy_only", {"VMV_TILE_RULES": "0"})):
                _ops._TUNED = {}
                os.environ.update(env)
                try:
                    if keep_eng is not None:
                        model._engines.pop(next((k for k in model._engines if k[2:4] == (32, 32)), None), None)
                    ms_x, _ = time_shape(32, 32)
                    ref_shape[tag + "_ms_per_step"] = round(ms_x, 3)
                finally:
                    for k in env:
                        os.environ.pop(k, None)
                    _ops._TUNED = keep_tab
            if keep_eng is not None:
                model._engines.pop(next((k for k in model._engines if k[2:4] == (32, 32)), None), None)
        except Exception as e:
            ref_shape = dict(ref_shape or {}, error=f"{type(e).__name__}: {e}")

    # ---- two prompts per plan (round 6): the reference denoises one prompt at a time; its sampler API admits noise [b, 4, F, h, w].  One
    #      sample's small levels do not fill 256 CUs, so b = 2 prompts in ONE plan of B = 4 row blocks (pair-major, fused CFG + DDIM update
    #      per sample: unet_t2v._forward_cfg_rows_batched) raise per-GPU throughput.  An extra object: `value` stays the 1-sample step.
    pbatch = None
    if rank == 0 and world == 1 and args.full and not args.no_op_profile and not args.no_prompt_batch:
        def time_batch(h, w, nb, n=8):
            x = torch.randn(nb, 4, args.frames, h, w, generator=g, device=dev)
            yb = torch.randn(nb, 77, 1024, generator=g, device=dev)
            kc_b, ku_b = dict(y=yb, camera_data=cam), dict(y=y0, camera_data=cam)
            for i in range(2):
                dif.ddim_step_hip(x, steps[i], model, kc_b, ku_b, 9.0, stride)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                dif.ddim_step_hip(x, steps[(2 + i) % len(steps)], model, kc_b, ku_b, 9.0, stride)
            torch.cuda.synchronize()
            return 1000.0 * (time.perf_counter() - t0) / n, bool(torch.isfinite(x).all())
        try:
            pbatch = dict(note="b prompts per plan (B = 2 b row blocks, pair-major; CFG prefix shared per prompt), same kernels and tile rule; "
                               "sample_steps_per_s = b / batched step; `value` above is the 1-prompt step; the t2v entrance's key: prompt_batch")
            for (h, w) in ([(H, W)] + ([(32, 32)] if (H, W) == (40, 64) else [])):
                ms1, _ = time_batch(h, w, 1)
                d = dict(ms_per_step_1_prompt=round(ms1, 3))
                for nb in ((2, 4) if h * w <= 1024 else (2,)):
                    msb, finb = time_batch(h, w, nb)
                    q = dict(ms_per_batched_step=round(msb, 3), sample_steps_per_s=round(1000.0 * nb / msb, 3),
                             throughput_vs_1_prompt=round(nb * ms1 / msb, 4), finite=finb)
                    if STEP_TFLOP.get((h, w)):
                        q["whole_step_frac_of_peak"] = round(nb * STEP_TFLOP[(h, w)] / (msb * 1e-3) / PEAK_MFMA16_TFLOPS, 4)
                    d[f"prompts_{nb}"] = q
                    if (h, w) == (32, 32) and nb == 2:
                        # where the gain comes from: the per-family table of the B = 4 plan beside the B = 2 plan's at the same shape
                        try:
                            fam4, _ = profile_plan(model.engine_for(4, args.frames, h, w, 77, dev, n_t=1, share_prefix=True))
                            fam2, _ = profile_plan(model.engine_for(2, args.frames, h, w, 77, dev, n_t=1, share_prefix=True))
                            q["families"], q["families_1_prompt"] = fam_table(fam4)[0], fam_table(fam2)[0]
                        except Exception as e:
                            q["families"] = dict(error=f"{type(e).__name__}: {e}")
                    for k_ in [k for k in getattr(model, "_engines", {}) if k[0] > 2]:      # (free the B > 2 engines' buffers)
                        model._engines.pop(k_, None)
                pbatch[f"{args.frames}x{h}x{w}"] = d
        except Exception as e:
            pbatch = dict(pbatch or {}, error=f"{type(e).__name__}: {e}")

    def headline():
        return {"metric": "denoise-steps/sec, t2v %dx%dx%d (latent %dx%dx%d), CFG 9.0, 50-step DDIM schedule" % (8 * H, 8 * W, args.frames, args.frames, H, W),
               "value": round(steps_per_s, 4), "unit": "denoise-steps/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": L.elem_name(), "data": "synthetic (seeded randn latents/text, real orbit cameras; random-init "
               "weights, zero-inits re-randomised)",
               "config": {"workload": f"t2v_infer.yaml UNetSD_T2VBase 1.413B, 24 views, latent {H}x{W}, 77 ctx tokens, "
                                      f"1 sample per GPU (cond+uncond batched)", "parallelism": f"replicas x{world}"},
               "rccl_ranks": rccl_ranks, "launcher": launcher, "pg_backend": (backend + (" (ranks share GPU 0: smoke test, not a measurement)" if share_gpu else "")) if dist is not None else None,
               "finite": finite, "roofline": roof, "reference_shape": ref_shape, "prompt_batch": pbatch}

    # ---- frame-parallel leg: ONE sample over all ranks (strong scaling of a sample's latency)
    fpar = None
    if fp_children:
        # default at N > 1: the leg runs in one child process per rank (run_fp_children: a fault there cannot cost the line below)
        fence()
        fpar = run_fp_children(args, rank, world, launcher, agreed_port())
        fence()
    elif args.full and dist is not None and args.frames % world == 0 and not args.no_frame_parallel:
        import threading
        done = threading.Event()
        state = {"stage": "init"}

        def watchdog():
            if not done.wait(args.frame_parallel_budget):
                if rank == 0:
                    out = headline()
                    out["frame_parallel"] = dict(state.get("partial") or {}, error=f"leg exceeded {args.frame_parallel_budget}s at "
                                                                               f"stage {state['stage']}")
                    print(json.dumps(out), flush=True)
                os._exit(0)

        threading.Thread(target=watchdog, daemon=True).start()
        try:
            from videomv_amd.comm import FrameComm
            comm = FrameComm()
            _OPEN_COMMS.append(comm)
            model.set_frame_parallel(comm)
            gs = torch.Generator(device=dev).manual_seed(11)       # the SAME sample on every rank
            noise_s = torch.randn(1, 4, args.frames, H, W, generator=gs, device=dev)
            ys, y0s = torch.randn(1, 77, 1024, generator=gs, device=dev), torch.randn(1, 77, 1024, generator=gs, device=dev)
            cams = cam
            fl = args.frames // world
            kc, ku = dict(y=ys, camera_data=cams), dict(y=y0s, camera_data=cams)

            def timed_leg(tag, srank=None, sworld=None):
                srank = rank if srank is None else srank
                fls = args.frames // (world if sworld is None else sworld)
                xs = noise_s[:, :, srank * fls:(srank + 1) * fls].clone().contiguous()
                state["stage"] = tag + ":warmup"
                for i in range(max(1, args.warmup)):
                    dif.ddim_step_hip(xs, steps[i % len(steps)], model, kc, ku, 9.0, stride)
                fence()
                state["stage"] = tag + ":timed"
                t0 = time.perf_counter()
                for i in range(args.steps):
                    dif.ddim_step_hip(xs, steps[(args.warmup + i) % len(steps)], model, kc, ku, 9.0, stride)
                fence()
                dtf = time.perf_counter() - t0
                tt = torch.tensor([dtf], device=cdev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                dtf = float(tt[0])
                r = dict(steps_per_s=round(args.steps / dtf, 4), ms_per_step=round(1000.0 * dtf / args.steps, 3),
                         finite=bool(torch.isfinite(xs).all()))
                if step_tflop:
                    r["whole_step_frac_of_peak"] = round(step_tflop * r["steps_per_s"] / world / PEAK_MFMA16_TFLOPS, 4)
                return r

            # the single-plan mode first (one B = 2 plan, one communicator), then the branch-pipelined default (two B = 1
            # plans on two streams, a communicator each): a problem in the second can never cost the first its number
            os.environ["VMV_FP_PIPELINE"] = "0"
            single = timed_leg("single-plan")
            eng = model.engine_for(2, args.frames, H, W, 77, dev, n_t=1)
            common = dict(scaling="strong", views_per_gpu=fl, collectives_per_branch_plan=len(eng.breaks) + eng.n_comm_ops,
                          collectives_issued_by=("C plan replay (VMV_OP_COMM, RCCL)" if eng.n_comm_ops else "Python (torch.distributed) between plan segments"),
                          all_to_all_per_step=sum(1 for lb in eng.S.labels if lb.endswith(".all_to_all")) + sum(1 for i, _ in eng.breaks if eng.S.labels[i].endswith(".unpack")),
                          parallelism=f"frames x{world} (frame-major <-> pixel-major all-to-all, DESIGN.md §8)")
            if comm._handle:         # the plan-recorded collectives' own RCCL communicator (csrc/comm.hip): ncclCommCount of it
                common["native_rccl_ranks"] = int(L.load().vmv_comm_world(comm._handle))
            state["partial"] = dict(common, mode="single-plan", **single)
            os.environ["VMV_FP_PIPELINE"] = "1"
            piped = timed_leg("branch-pipelined")
            best, mode = (piped, "branch-pipelined") if piped["steps_per_s"] >= single["steps_per_s"] else (single, "single-plan")
            fpar = dict(common, mode=mode, **best, single_plan=single, branch_pipelined=piped)
            state["partial"] = dict(fpar)
            if world % 2 == 0 and args.frames % (world // 2) == 0:
                # CFG-parallel x frame-parallel: one branch per half of the ranks, frames sharded world/2 ways inside each half
                from videomv_amd.comm import CfgFrameComm
                state["stage"] = "cfg-parallel:groups"
                comm2 = CfgFrameComm()
                _OPEN_COMMS.append(comm2)
                model.set_frame_parallel(comm2)
                cfgp = timed_leg("cfg-parallel", comm2.rank, comm2.world)
                fpar["cfg_x_frame"] = dict(cfgp, parallelism=f"2 branch groups x {comm2.world} frame shards")
                if cfgp["steps_per_s"] > fpar["steps_per_s"]:
                    fpar.update(cfgp, mode="cfg-parallel x frame-parallel")
            # the branch-pipelined mode again with each branch plan replayed as ONE hipGraph (kernels + RCCL collectives captured
            # together, VMV_GRAPH=1) — meaningful only when the collectives are plan ops; inside its own try
            state["partial"] = dict(fpar)
            if eng.n_comm_ops:
                try:
                    os.environ["VMV_GRAPH"], os.environ["VMV_FP_PIPELINE"] = "1", "1"
                    model.set_frame_parallel(comm)
                    fpar["branch_pipelined_graph"] = timed_leg("pipelined+graph")
                except Exception as e:
                    fpar["branch_pipelined_graph"] = dict(error=f"{type(e).__name__}: {e}")
                finally:
                    os.environ.pop("VMV_GRAPH", None)
            # BASELINE's north-star form of configs[2], measured beside the default: frames stay sharded through the temporal
            # transformers, one all-gather of [K | V] before each temporal attention (VMV_FP_TEMPORAL=kv_gather; branch-pipelined
            # B = 1 plans).  Last, inside its own try: nothing above depends on it.
            state["partial"] = dict(fpar)
            try:
                os.environ["VMV_FP_TEMPORAL"], os.environ["VMV_FP_PIPELINE"] = "kv_gather", "1"
                model.set_frame_parallel(comm)
                kvg = timed_leg("kv-gather")
                fpar["kv_gather_temporal"] = dict(kvg, parallelism=f"frames x{world}, K|V all-gather per temporal attention (north-star form)")
            except Exception as e:
                fpar["kv_gather_temporal"] = dict(error=f"{type(e).__name__}: {e}")
            finally:
                os.environ.pop("VMV_FP_TEMPORAL", None)
            # b prompts per plan over the group (round 6): the ranks' launch-bound 1 / W shares get b times the rows.  Single plan,
            # plain FrameComm; per-sample latency = the batched step, group throughput = b / batched step.  Last, inside its own try.
            state["partial"] = dict(fpar)
            if not args.no_prompt_batch:
                try:
                    os.environ["VMV_FP_PIPELINE"] = "0"
                    model.set_frame_parallel(comm)
                    fpar["prompts_per_plan"] = {}
                    for nb in (2, 4):
                        state["stage"] = f"prompts-{nb}:warmup"
                        xb = torch.randn(nb, 4, args.frames, H, W, generator=gs, device=dev)[:, :, rank * fl:(rank + 1) * fl].contiguous()
                        kcb = dict(y=torch.randn(nb, 77, 1024, generator=gs, device=dev), camera_data=cams)
                        for i in range(max(1, args.warmup)):
                            dif.ddim_step_hip(xb, steps[i % len(steps)], model, kcb, ku, 9.0, stride)
                        fence()
                        state["stage"] = f"prompts-{nb}:timed"
                        t0 = time.perf_counter()
                        for i in range(args.steps):
                            dif.ddim_step_hip(xb, steps[(args.warmup + i) % len(steps)], model, kcb, ku, 9.0, stride)
                        fence()
                        tt = torch.tensor([time.perf_counter() - t0], device=cdev)
                        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                        tb = float(tt[0]) / args.steps
                        fpar["prompts_per_plan"][str(nb)] = dict(ms_per_batched_step=round(1000 * tb, 3), ms_per_sample_step=round(1000 * tb / nb, 3),
                                                                 group_sample_steps_per_s=round(nb / tb, 3), finite=bool(torch.isfinite(xb).all()))
                except Exception as e:
                    fpar["prompts_per_plan"] = dict(fpar.get("prompts_per_plan") or {}, error=f"{type(e).__name__}: {e}")
        except Exception as e:      # the headline (replicas) line must survive any problem in this leg
            fpar = dict(state.get("partial") or {}, error=f"{type(e).__name__}: {e}")
        finally:
            os.environ.pop("VMV_FP_PIPELINE", None)
            model.set_frame_parallel(None)
            done.set()

    # ---- one complete 24-view sample: 50 DDIM steps + VAE decode of 24 frames in chunks of decoder_bs = 4
    sample = None
    if rank == 0 and world == 1 and args.full and not args.no_sample:
        from videomv_amd.registry import AUTO_ENCODER
        import videomv_amd.autoencoder  # noqa: F401
        from videomv_amd.pipeline import sample_views, decode_views
        dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                  num_res_blocks=2, attn_resolutions=[], dropout=0.0)
        with torch.device(dev):
            vae = AUTO_ENCODER.build(dict(type="AutoencoderKL", ddconfig=dd, embed_dim=4))
        randomize_(vae, 4321)
        decode_views(vae, noise)                     # warm-up: builds the decoder plan
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        x0_lat, _ = sample_views(model, dif, vae, noise, y, y0, cam, guide_scale=9.0, ddim_timesteps=50, decode=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        vid = decode_views(vae, x0_lat, decoder_bs=4)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        sample = dict(seconds=round(t3 - t1, 4), ddim50_seconds=round(t2 - t1, 4), vae_decode24_seconds=round(t3 - t2, 4),
                      samples_per_s=round(1.0 / (t3 - t1), 5), video_shape=list(vid.shape),
                      finite=bool(torch.isfinite(vid).all() and torch.isfinite(x0_lat).all()))
        if not args.no_prompt_batch:       # the same, two prompts per plan (the entrance's `prompt_batch: 2`): 2 samples per pass
            try:
                n2 = torch.randn(2, 4, args.frames, H, W, generator=g, device=dev)
                y2 = torch.randn(2, 77, 1024, generator=g, device=dev)
                y02 = y0.expand(2, -1, -1).contiguous()
                sample_views(model, dif, vae, n2, y2, y02, cam, guide_scale=9.0, ddim_timesteps=2, decode=False)      # (records the B = 4 plan)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                x0_2, vid2 = sample_views(model, dif, vae, n2, y2, y02, cam, guide_scale=9.0, ddim_timesteps=50, decoder_bs=4)
                torch.cuda.synchronize()
                t5 = time.perf_counter()
                sample["two_prompts_per_plan"] = dict(seconds_for_2_samples=round(t5 - t4, 4), samples_per_s=round(2.0 / (t5 - t4), 5),
                                                      vs_one_prompt=round(2.0 * (t3 - t1) / (t5 - t4), 4), video_shape=list(vid2.shape),
                                                      finite=bool(torch.isfinite(vid2).all() and torch.isfinite(x0_2).all()))
                del x0_2, vid2
                for k_ in [k for k in getattr(model, "_engines", {}) if k[0] == 4]:
                    model._engines.pop(k_, None)
            except Exception as e:
                sample["two_prompts_per_plan"] = dict(error=f"{type(e).__name__}: {e}")

    # ---- the once-per-prompt conditioning upstream of the loop: open_clip ViT-H/14 text (2 prompts: caption + negative) and image
    #      towers on the same kernels (clip_embedder.py:187-201); full-size, random-init on the device
    clip = None
    if rank == 0 and world == 1 and args.full and not args.no_sample:
        try:
            from videomv_amd.clip_text import ClipTextEngine, ClipTextOptions, clip_text_shapes
            from videomv_amd.clip_vision import ClipVisionEngine, ClipVisionOptions, clip_vision_shapes

            def rand_sd(shapes, seed):
                gg = torch.Generator(device=dev).manual_seed(seed)
                sd = {}
                for k, shp in shapes.items():
                    t = torch.randn(shp, device=dev, generator=gg)
                    is_ln = (".ln_" in k or k.startswith("ln_") or "ln_p" in k) and k.endswith(".weight")
                    sd[k] = 1 + 0.1 * t if is_ln else 0.05 * t if k.endswith("bias") else 0.5 * t if "embedding" in k else t * shp[-1] ** -0.5
                return sd

            def time_plan(eng, reps=5):
                eng.S.run(); torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    eng.S.run()
                b.record(); torch.cuda.synchronize()
                return a.elapsed_time(b) / reps
            ot, ov = ClipTextOptions(), ClipVisionOptions()
            te = ClipTextEngine(ot, rand_sd(clip_text_shapes(ot), 5), 2, dev, layer_idx=1)
            tok = torch.zeros(2, 77, dtype=torch.long, device=dev); tok[:, 0] = 49406; tok[0, 1:6] = torch.arange(320, 325, device=dev); tok[0, 6] = 49407; tok[1, 1] = 49407
            xt, xw = te.forward(tok)
            t_text = time_plan(te)
            ve = ClipVisionEngine(ov, rand_sd(clip_vision_shapes(ov), 6), 1, dev)
            yv = ve.forward(torch.randn(1, 3, 224, 224, device=dev))
            t_img = time_plan(ve)
            clip = dict(text_tower_ms=round(t_text, 3), text_prompts=2, text_launches=te.S.nops, image_tower_ms=round(t_img, 3), image_launches=ve.S.nops,
                        arch="open_clip ViT-H-14 (text 354 M, penultimate layer; visual 632 M), random-init", y_words=list(xw.shape), y_visual=list(yv.shape),
                        finite=bool(torch.isfinite(xw).all() and torch.isfinite(yv).all()))
            del te, ve
            torch.cuda.empty_cache()
        except Exception as e:      # (reported, never fatal to the headline)
            clip = {"error": f"{type(e).__name__}: {e}"}

    # ---- BASELINE configs[4]: one LGM-refined sample at the reference's own 256-px shape (latent 24x32x32): 50 DDIM steps,
    #      of which steps 20/30/40 send each CFG branch through VAE decode (4 views) -> LGM U-Net (415 M) -> 65 536
    #      Gaussians -> 24 renders at 512^2 -> VAE encode (24 views); full-size LGM, random weights
    lgm = None
    if rank == 0 and world == 1 and args.full and not args.no_sample and not args.no_lgm:
        from videomv_amd.lgm import prepare_gs_data
        from videomv_amd.camera import entrance_camera_data
        with torch.device(dev):
            model_l = MODEL.build(dict(type="UNetSD_T2VBase", y_dim=1024, use_camera_condition=True, use_lgm_refine=True, **FULL))
        randomize_(model_l, 1234)
        model_l.eval()
        cam_l = entrance_camera_data(24, elevation=15, camera_distance=2.0)
        gs_data = prepare_gs_data(cam_l, model_l.lgm_opt)
        gl = torch.Generator(device=dev).manual_seed(11)
        noise_l = torch.randn(1, 4, 24, 32, 32, generator=gl, device=dev)
        kw_l = [dict(y=y, camera_data=cam_l, gs_data=gs_data), dict(y=y0, camera_data=cam_l, gs_data=gs_data)]
        xl = noise_l.clone()
        dif.ddim_step_hip(xl, steps[0], model_l, kw_l[0], kw_l[1], 9.0, stride)          # warm-up: plans, VAE engines, LGM
        # the LGM-refined step: 2 warm-up calls, then 6 timed ones (round 2 timed ONE call after one warm-up and the driver's box
        # recorded it cold: 138 ms against ~80 in the loop); median and min are reported, next to the in-loop figure below
        for i in range(2):
            dif.ddim_step_lgm(xl, steps[1 + i], model_l, kw_l[0], kw_l[1], 9.0, stride, vae)
        t_calls = []
        for i in range(6):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dif.ddim_step_lgm(xl, steps[3 + i], model_l, kw_l[0], kw_l[1], 9.0, stride, vae)
            torch.cuda.synchronize()
            t_calls.append(time.perf_counter() - t1)
        t_calls.sort()
        t_lgm_step, t_lgm_min = 0.5 * (t_calls[2] + t_calls[3]), t_calls[0]
        # plain steps at this shape (for the in-loop attribution: loop = 47 plain + 3 refined steps)
        xp = noise_l.clone()
        for i in range(2):
            dif.ddim_step_hip(xp, steps[i], model_l, kw_l[0], kw_l[1], 9.0, stride)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(8):
            dif.ddim_step_hip(xp, steps[2 + i], model_l, kw_l[0], kw_l[1], 9.0, stride)
        torch.cuda.synchronize()
        t_plain = (time.perf_counter() - t1) / 8
        t1 = time.perf_counter()
        x0_l = dif.ddim_sample_loop(noise=noise_l, model=model_l, autoencoder=vae, model_kwargs=kw_l, guide_scale=9.0,
                                    ddim_timesteps=50, eta=0.0)
        torch.cuda.synchronize()
        t_loop = time.perf_counter() - t1
        ref_l = model_l.lgm_refiner(dev)
        lgm = dict(workload="t2v + use_lgm_refine=True, latent 24x32x32, 50 DDIM steps, LGM at step indices 20/30/40 "
                            "(2 branches each): LGM 'big' 415 M params, 65 536 Gaussians, 24 renders at 512x512 per branch",
                   ddim50_lgm_seconds=round(t_loop, 4), lgm_refined_step_ms=round(1000 * t_lgm_step, 2),
                   lgm_refined_step_min_ms=round(1000 * t_lgm_min, 2), lgm_refined_step_calls=6,
                   plain_step_ms=round(1000 * t_plain, 2),
                   lgm_refined_step_in_loop_ms=round(1000 * (t_loop - 47 * t_plain) / 3, 2),
                   instances_per_view=int(sum(ref_l.renderer.last_num_rendered) / max(1, getattr(ref_l.renderer, "last_views", 0) or len(ref_l.renderer.last_num_rendered))),
                   finite=bool(torch.isfinite(x0_l).all()))
        if not args.no_prompt_batch:      # the same refined loop with two prompts per plan (the YAML default use_lgm_refine + `prompt_batch: 2`):
            try:                          # 47 plain steps batched, the 3 refined ones sample by sample
                n2l = torch.randn(2, 4, 24, 32, 32, generator=gl, device=dev)
                kw2 = [dict(y=torch.randn(2, 77, 1024, generator=gl, device=dev), camera_data=cam_l, gs_data=gs_data),
                       dict(y=y0.expand(2, -1, -1).contiguous(), camera_data=cam_l, gs_data=gs_data)]
                dif.ddim_sample_loop(noise=n2l, model=model_l, model_kwargs=kw2[:1] + [dict(kw2[1])], guide_scale=9.0, ddim_timesteps=2, eta=0.0)   # (records the B = 4 plan)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                x0_2l = dif.ddim_sample_loop(noise=n2l, model=model_l, autoencoder=vae, model_kwargs=kw2, guide_scale=9.0, ddim_timesteps=50, eta=0.0)
                torch.cuda.synchronize()
                t2l = time.perf_counter() - t1
                lgm["two_prompts_per_plan"] = dict(ddim50_lgm_seconds_for_2_samples=round(t2l, 4), samples_per_s=round(2.0 / t2l, 4),
                                                   vs_one_prompt=round(2.0 * t_loop / t2l, 4), finite=bool(torch.isfinite(x0_2l).all()))
                del x0_2l
            except Exception as e:
                lgm["two_prompts_per_plan"] = dict(error=f"{type(e).__name__}: {e}")
        del model_l

    # ---- the rasteriser alone on the last refined step's Gaussians (BASELINE configs[4]'s only new kernel family): HBM-bound,
    #      DESIGN.md §4.4's algorithmic bytes = 48 B per Gaussian (14 fp32 attributes read once, the per-Gaussian screen-space
    #      record written) + 12 B per (tile, Gaussian) instance (64-bit key + index written; sort passes and blend reads not
    #      counted) + 16 B per pixel written, per view
    if lgm is not None and ref_l.last_gaussians is not None:
        try:
            gsn = ref_l.last_gaussians.unsqueeze(0).contiguous()
            cv, cvp = gs_data["cam_view"].to(dev), gs_data["cam_view_proj"].to(dev)
            ref_l.renderer.render(gsn, cv, cvp, None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(3):
                ref_l.renderer.render(gsn, cv, cvp, None)
            torch.cuda.synchronize()
            t_r = (time.perf_counter() - t1) / 3
            nview, S_out = cv.shape[1], ref_l.renderer.size
            inst = sum(ref_l.renderer.last_num_rendered)
            by = nview * (gsn.shape[1] * 48 + S_out * S_out * 16) + inst * 12
            # same-run A/B: the per-view loop of round 4 (one host round trip per view)
            os.environ["VMV_GS_BATCH"] = "0"
            try:
                ref_l.renderer.render(gsn, cv, cvp, None)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(3):
                    ref_l.renderer.render(gsn, cv, cvp, None)
                torch.cuda.synchronize()
                t_pv = (time.perf_counter() - t1) / 3
            finally:
                os.environ.pop("VMV_GS_BATCH", None)
            lgm["rasteriser"] = dict(views=nview, gaussians=int(gsn.shape[1]), instances=int(inst), ms_per_24_views=round(1000 * t_r, 3),
                                     ms_per_view=round(1000 * t_r / nview, 4), algorithmic_bytes=int(by),
                                     achieved_gb_s=round(by / t_r / 1e9, 1), peak_gb_s=8000.0, frac=round(by / t_r / 8e12, 4),
                                     per_view_loop_ms_per_24_views=round(1000 * t_pv, 3), host_syncs_per_call=1,
                                     bound="valu (the blend: ~8 G pixel x Gaussian evaluations per 24 views at 13-30 vector instructions each is "
                                           "56 % of the GPU time in profiles/r6_gs_kernel_stats_after.txt; the HBM figure is kept for continuity, it is "
                                           "not what limits the pass)",
                                     note="wall time of GaussianRenderer.render: ONE batched pass over all views (preprocess, per-view depth ranking, "
                                          "scan, ONE host read of the instance total, coalesced duplicate, 2-pass radix sort on the 32-bit tile id, "
                                          "ranges, branch-free blend — round 6); per_view_loop = round 4's loop with a host round trip per view and "
                                          "the 64-bit (tile, depth) sort, same run, same bits")
        except Exception as e:
            lgm["rasteriser"] = {"error": f"{type(e).__name__}: {e}"}
    if lgm is not None:
        del ref_l

    # ---- BASELINE configs[3]: the full-size UNetSD_I2VGen (1.422 B parameters: the T2V trunk with an 8-channel input conv + the image
    #      front-end), 24 views, 77 text + 64 local-image + 4 CLIP-image = 145 context tokens, v-prediction on the cosine /
    #      zero-terminal-SNR schedule, guide 6 (i2vgen_xl_infer.yaml) — at the config's own 256-px shape (latent 32x32) and at the
    #      headline's 320x512 (latent 40x64)
    i2v = None
    if rank == 0 and world == 1 and args.full and not args.no_sample and not args.no_i2vgen:
        try:
            import videomv_amd.unet_i2vgen  # noqa: F401
            with torch.device(dev):
                m_i = MODEL.build(dict(type="UNetSD_I2VGen", y_dim=1024, concat_dim=4, use_camera_condition=True, use_lgm_refine=False, **FULL))
            randomize_(m_i, 4242)
            m_i.eval()
            dif_v = DIFFUSION.build(dict(type="DiffusionDDIM", schedule="cosine",
                                         schedule_param=dict(num_timesteps=1000, cosine_s=0.008, zero_terminal_snr=True),
                                         mean_type="v", var_type="fixed_small"))
            steps_v = [int(v) for v in dif_v.ddim_steps(50)]
            gi = torch.Generator(device=dev).manual_seed(9999)          # i2vgen_xl_infer.yaml seed
            img, img0 = torch.randn(1, 1, 1024, generator=gi, device=dev), torch.zeros(1, 1, 1024, device=dev)
            fps = torch.tensor([8], device=dev)
            i2v = dict(workload="i2vgen_xl_infer.yaml UNetSD_I2VGen, 24 views, 145 ctx tokens (77 text + 64 local-image + 4 CLIP-image), "
                                "v-prediction, cosine schedule with zero terminal SNR, CFG 6.0, cond + uncond batched",
                       params=int(sum(p_.numel() for p_ in m_i.parameters())), shapes={})
            for hh, ww in ((32, 32), (H, W)):
                noise_i = torch.randn(1, 4, args.frames, hh, ww, generator=gi, device=dev)
                li = torch.randn(1, 4, hh, ww, generator=gi, device=dev).unsqueeze(2).repeat_interleave(args.frames, dim=2)
                kci = dict(y=y, image=img, local_image=li, fps=fps, camera_data=cam)
                kui = dict(y=y0, image=img0, local_image=li, fps=fps, camera_data=cam)
                xi = noise_i.clone()
                for i in range(max(2, args.warmup)):
                    dif_v.ddim_step_hip(xi, steps_v[1 + i], m_i, kci, kui, 6.0, stride)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for i in range(args.steps):
                    dif_v.ddim_step_hip(xi, steps_v[(3 + i) % 49 + 1], m_i, kci, kui, 6.0, stride)
                torch.cuda.synchronize()
                t_i = (time.perf_counter() - t1) / args.steps
                r = dict(ms_per_step=round(1000 * t_i, 3), steps_per_s=round(1.0 / t_i, 4), finite=bool(torch.isfinite(xi).all()))
                tf = STEP_TFLOP.get((hh, ww))
                if tf:       # (the T2V trunk's algorithmic FLOPs: the 8-channel input conv and the 68 extra context tokens add < 1 %)
                    r["whole_step"] = dict(algorithmic_tflop=tf, achieved=round(tf / t_i, 1), frac=round(tf / t_i / PEAK_MFMA16_TFLOPS, 4))
                if not args.no_prompt_batch:       # two input images per plan (round 6: B = 4 row blocks, pair-major; unet_i2vgen._forward_cfg_rows_batched)
                    try:
                        xb = torch.randn(2, 4, args.frames, hh, ww, generator=gi, device=dev)
                        lib = torch.randn(2, 4, hh, ww, generator=gi, device=dev).unsqueeze(2).repeat_interleave(args.frames, dim=2)
                        yb, imb = torch.randn(2, 77, 1024, generator=gi, device=dev), torch.randn(2, 1, 1024, generator=gi, device=dev)
                        kcb = dict(y=yb, image=imb, local_image=lib, fps=fps, camera_data=cam)
                        kub = dict(y=y0, image=img0, local_image=lib, fps=fps, camera_data=cam)
                        for i in range(2):
                            dif_v.ddim_step_hip(xb, steps_v[1 + i], m_i, kcb, kub, 6.0, stride)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        for i in range(args.steps):
                            dif_v.ddim_step_hip(xb, steps_v[(3 + i) % 49 + 1], m_i, kcb, kub, 6.0, stride)
                        torch.cuda.synchronize()
                        t_b = (time.perf_counter() - t1) / args.steps
                        r["two_images_per_plan"] = dict(ms_per_batched_step=round(1000 * t_b, 3), sample_steps_per_s=round(2.0 / t_b, 3),
                                                        throughput_vs_1_image=round(2.0 * t_i / t_b, 4), finite=bool(torch.isfinite(xb).all()))
                        for k_ in [k for k in getattr(m_i, "_engines", {}) if k[0] > 2]:
                            m_i._engines.pop(k_, None)
                    except Exception as e:
                        r["two_images_per_plan"] = dict(error=f"{type(e).__name__}: {e}")
                i2v["shapes"][f"{args.frames}x{hh}x{ww}"] = r
            del m_i
            torch.cuda.empty_cache()
        except Exception as e:
            i2v = dict(i2v or {}, error=f"{type(e).__name__}: {e}")

    # ---- BASELINE configs[2] on ONE GPU: rank 0's plan of a W-GPU frame-parallel run with the W - 1 peers simulated (comm.SimComm:
    #      every collective a device-local copy of the same bytes, issued from the C replay loop like the RCCL ones).  GPU ms per
    #      step = this rank's kernels + local copies (no wire time: the xGMI floor of its bytes is reported beside it); host ms per
    #      step = the time the Python thread needs to enqueue one step.  NOT a sample (peers' data = this rank's own).
    simr = None
    if rank == 0 and world == 1 and args.full and args.simulate_rank > 1 and args.frames % args.simulate_rank == 0:
        Wn = args.simulate_rank
        try:
            from videomv_amd.comm import SimComm
            fl = args.frames // Wn
            xs0 = noise[:, :, :fl].clone().contiguous()
            simr = dict(world=Wn, rank=0, views_per_gpu=fl, plain_step_ms_this_box=round(ms_per_step, 3),
                        note="peers simulated on one GPU: kernels, tiles, local copies and host time are the real rank's; wire time is not included "
                             "and the output is not a sample", modes={})

            def sim_leg(pipeline, graph, cfgpar=False):
                os.environ["VMV_FP_PIPELINE"], os.environ["VMV_GRAPH"] = ("1" if pipeline else "0"), ("1" if graph else "0")
                if cfgpar:       # 2 branch groups of Wn / 2 ranks: this rank runs ONE B = 1 plan on 2 * frames / Wn views
                    from videomv_amd.comm import SimCfgFrameComm
                    model.set_frame_parallel(SimCfgFrameComm(Wn))
                    xs = noise[:, :, :2 * fl].clone().contiguous()
                else:
                    model.set_frame_parallel(SimComm(Wn, 0))
                    xs = xs0.clone()
                for i in range(3):                                   # eager, capture, first graph launch
                    dif.ddim_step_hip(xs, steps[i % len(steps)], model, kw_c, kw_u, 9.0, stride)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for i in range(args.steps):
                    dif.ddim_step_hip(xs, steps[(3 + i) % len(steps)], model, kw_c, kw_u, 9.0, stride)
                t_host_all = time.perf_counter() - t1
                torch.cuda.synchronize()
                t_all = time.perf_counter() - t1
                hs = []
                for i in range(5):                                   # host time of ONE step's enqueue on an idle queue
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    dif.ddim_step_hip(xs, steps[(7 + i) % len(steps)], model, kw_c, kw_u, 9.0, stride)
                    hs.append(time.perf_counter() - t1)
                torch.cuda.synchronize()
                engs = model._pipe["engs"] if ((pipeline or cfgpar) and model._pipe) else [model.engine_for(2, args.frames, H, W, 77, dev, n_t=1, share_prefix=True)]
                e0 = engs[0]
                ncoll = sum(e.n_comm_ops for e in engs)
                bytes_in = sum(e.comm_bytes_in for e in engs)
                r = dict(gpu_ms_per_step=round(1000 * t_all / args.steps, 3), host_ms_per_step=round(1000 * sorted(hs)[len(hs) // 2], 3),
                         host_ms_per_step_queued=round(1000 * t_host_all / args.steps, 3),
                         launches_per_step=sum(e.S.nops for e in engs), collectives_per_step=ncoll, python_collectives_per_step=sum(len(e.breaks) for e in engs),
                         bytes_received_per_step=int(bytes_in),
                         xgmi_floor_ms=round(1000 * bytes_in / (7 * 76.8e9), 3),
                         graph=bool(graph and all(e.S.graph for e in engs)), graph_nodes=[e.graph_nodes for e in engs] if graph else None,
                         finite=bool(torch.isfinite(xs).all()))
                if step_tflop:
                    r["frac_of_peak_if_all_ranks_equal"] = round(step_tflop / Wn / (t_all / args.steps) / PEAK_MFMA16_TFLOPS, 4)
                return r, e0

            legs = [("single-plan", 0, 0, False), ("branch-pipelined", 1, 0, False)]
            if Wn % 2 == 0 and args.frames % (Wn // 2) == 0:
                legs.append((f"cfg x frame (2 x {Wn // 2})", 0, 0, True))         # half the launches per rank
            for tag, pl, gr, cp in legs:
                try:
                    simr["modes"][tag], e0 = sim_leg(pl, gr, cp)
                    if tag == "single-plan":          # per-family table of the rank-local B = 2 plan (tile policy at M / W)
                        fam_s, _ = profile_plan(e0, dump=args.dump_ops_sim)
                        simr["families_single_plan"], simr["serial_forward_ms"] = fam_table(fam_s)
                        simr["serial_forward_ms"] = round(simr["serial_forward_ms"], 3)
                except Exception as e:
                    simr["modes"][tag] = {"error": f"{type(e).__name__}: {e}"}
            # b prompts per plan ON the simulated rank (round 6): a rank's 1 / W share of ONE sample is launch-bound (~1 100 dependent launches
            # of ~15 us for 1 / W of the FLOPs); with b prompts in the plan the launches stay and their rows grow b-fold.  Single-plan mode.
            if not args.no_prompt_batch:
                simr["prompts_per_plan"] = {}
                for nb in (2, 4, 8):
                    try:
                        os.environ["VMV_FP_PIPELINE"], os.environ["VMV_GRAPH"] = "0", "0"
                        model.set_frame_parallel(SimComm(Wn, 0))
                        xb = torch.randn(nb, 4, fl, H, W, generator=g, device=dev)
                        kcb = dict(y=torch.randn(nb, 77, 1024, generator=g, device=dev), camera_data=cam)
                        for i in range(2):
                            dif.ddim_step_hip(xb, steps[i % len(steps)], model, kcb, kw_u, 9.0, stride)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        for i in range(args.steps):
                            dif.ddim_step_hip(xb, steps[(2 + i) % len(steps)], model, kcb, kw_u, 9.0, stride)
                        torch.cuda.synchronize()
                        tb = (time.perf_counter() - t1) / args.steps
                        q_ = dict(gpu_ms_per_batched_step=round(1000 * tb, 3), gpu_ms_per_sample_step=round(1000 * tb / nb, 3),
                                  group_sample_steps_per_s_no_wire=round(nb / tb, 2), replicas_sample_steps_per_s=round(Wn * steps_per_s, 2),
                                  finite=bool(torch.isfinite(xb).all()))
                        if step_tflop:
                            q_["frac_of_peak_if_all_ranks_equal"] = round(nb * step_tflop / Wn / tb / PEAK_MFMA16_TFLOPS, 4)
                        simr["prompts_per_plan"][str(nb)] = q_
                    except Exception as e:
                        simr["prompts_per_plan"][str(nb)] = {"error": f"{type(e).__name__}: {e}"}
                    finally:
                        for k_ in [k for k in getattr(model, "_engines", {}) if k[0] > 2]:
                            model._engines.pop(k_, None)
            best = min((v["gpu_ms_per_step"], k) for k, v in simr["modes"].items() if "gpu_ms_per_step" in v)
            simr["best_mode"], simr["best_gpu_ms_per_step"] = best[1], best[0]
            simr["projected_speedup_vs_1gpu_no_wire"] = round(ms_per_step / best[0], 2)
        except Exception as e:
            simr = dict(simr or {}, error=f"{type(e).__name__}: {e}")
        finally:
            os.environ.pop("VMV_FP_PIPELINE", None); os.environ.pop("VMV_GRAPH", None)
            model.set_frame_parallel(None)

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cores = os.cpu_count() or 1
        try:
            cores = len(os.sched_getaffinity(0))
        except Exception:
            pass
        # Two thread counts: the host's PHYSICAL cores — the baseline SURVEY §8d defines — and 64, where torch-CPU
        # eager stops scaling on these shapes; both are reported, `value` is the faster of the two (the baseline at its best).
        phys = physical_cores(cores)
        runs = []
        t_cpu0 = time.time()
        # (64 threads first — the leg `value` normally comes from; the physical-cores leg gets what is left of a ~250-s total (round 6: enough
        #  for the bench shape itself on the 128-core hosts of the pool, 77 s there: VERDICT r5 weak #13), and steps
        #  down to the reference's 32x32 shape when the bench shape is predicted not to fit: its `latent` says which one ran)
        for th in sorted({phys, min(cores, 64)}, key=lambda v: (v != min(cores, 64), v)):
            left = max(40.0, 250.0 - (time.time() - t_cpu0)) if runs else CPU_BUDGET_S
            r = cpu_baseline(args.frames, cores, (H, W), threads=th, budget=left)
            runs.append(dict(threads=r[1], s_per_forward=None if r[0] is None else round(r[0], 2),
                             latent=None if r[2] is None else f"{args.frames}x{r[2][0]}x{r[2][1]}", _r=r))
        full = [q for q in runs if q["_r"][0] is not None and q["_r"][2] == (H, W)] or [q for q in runs if q["_r"][0] is not None]
        t_fwd, threads, shp = min(full, key=lambda q: q["_r"][0])["_r"] if full else (None, runs[0]["threads"], None)
        for q in runs:
            q.pop("_r")
        if t_fwd is not None:
            ch, cw = shp
            same = (ch, cw) == (H, W)
            cpu = dict(value=round(1.0 / (2.0 * t_fwd), 6), unit="denoise-steps/s", cores=threads, kind="port",
                       latent=f"{args.frames}x{ch}x{cw}", same_shape_as_bench=same, host_cores=cores, physical_cores=phys, runs=runs,
                       sample=f"1 oracle UNet forward (fp32 torch-CPU eager, full-size 1.413B weights) at latent "
                              f"{args.frames}x{ch}x{cw}: {t_fwd:.2f} s on {threads} threads of {cores} host cores; a step = 2 "
                              f"forwards (cond + uncond), so value = 1 / (2 x {t_fwd:.2f} s); no scaling"
                              + ("" if same else f" — NOT the bench shape {H}x{W}: it did not finish inside the budget there"))
        else:
            cpu = dict(value=None, unit="denoise-steps/s", cores=threads, kind="port", host_cores=cores, physical_cores=phys, runs=runs,
                       sample="oracle forward did not finish inside the budget at any rung of the ladder")

    # ---- the same timed region with the OTHER element type's kernels (child process: a process loads one library).  BASELINE
    #      configs[1] says bf16; the default is fp16 because only fp16 meets the stated parity tolerances
    alt = None
    if rank == 0 and world == 1 and args.full and args.alt_dtype and not args.no_alt_dtype and not args.no_sample:
        import subprocess
        other = "bf16" if L.elem_name() == "fp16" else "fp16"
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--latent",
               args.latent, "--frames", str(args.frames), "--no-cpu-baseline", "--no-sample", "--no-lgm", "--no-op-profile",
               "--no-alt-dtype"]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240, env=dict(os.environ, VMV_DTYPE=other))
            line = next((l for l in r.stdout.splitlines() if l.startswith("{")), None)
            if line:
                dj = json.loads(line)
                alt = dict(dtype=dj["dtype"], value=dj["value"], ms_per_step=dj["ms_per_step"], finite=dj["finite"],
                           parity=("meets SURVEY 8d (1e-2 / 5e-3 / 2e-2)" if other == "fp16" else
                                   "does NOT meet SURVEY 8d: 1.3e-2 per forward, held to 3e-2 / 3e-2 / 6e-2 in the tests"))
        except Exception as e:
            alt = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        out = headline()
        out.update({"sample_24view": sample, "clip_towers": clip, "lgm_refined_sample": lgm, "i2vgen": i2v, "frame_parallel": fpar,
                    "simulated_rank": simr, "cpu_baseline": cpu})
        if alt is not None:
            out["other_dtype"] = alt
        print(json.dumps(out), flush=True)
    if dist is not None:
        for c in _OPEN_COMMS:       # native RCCL communicators first (collective: every rank built the same ones)
            try:
                c.close()
            except Exception:
                pass
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
