"""``GaussianFitter`` — fits a fixed set of 3-D Gaussians to a view set on the gfx950 rasteriser and its backward pass
(``csrc/raster.hip`` + ``csrc/raster_bwd.hip``, contract: ``include/vmv.h`` "Fitting Gaussians to a view set").

The reference's last stage, reconstruction from the generated views, is unreleased (its README lists it as to-do); its LGM trains
on an image MSE (``core/models.py:169``) and exports with ``save_ply`` (``core/gs.py:97``).  Here the LGM's feed-forward Gaussians
of the final sample are the starting point and every generated view is a target.  One iteration on one stream: batched preprocess
-> ONE host read of the instance total -> forward with saved state -> loss + dL/dimage -> blend backward -> preprocess backward and
view sum -> fused Adam step on the raw parameters (logit opacity, log scale, raw quaternion, SH-DC colour: the .ply layout), which
writes the activated Gaussians the next forward reads.  N stays fixed (no densification or pruning).

The loss is the image MSE (``loss="mse"``, the default) or the objective of 3-D Gaussian Splatting, ``(1 - lambda) L1 + lambda
(1 - SSIM)`` (``loss="l1_dssim"``, ``csrc/gs_ssim.hip``); ``ssim()`` is that kernel's forward as a metric.
"""
import ctypes as C
import math
import time

import torch

from . import _lib as L
from .gs import GaussianRenderer
from .ops import _stream_ptr

SH_C0 = 0.28209479177387814
# per-group learning rates of 3-D Gaussian Splatting (Kerbl et al. 2023, arguments.py: position 1.6e-4 x the scene extent, feature
# 2.5e-3, opacity 5e-2, scaling 5e-3, rotation 1e-3), the position group multiplied by the extent of the cameras
DEFAULT_LR = dict(position=1.6e-4, opacity=5e-2, scale=5e-3, rotation=1e-3, colour=2.5e-3)


def gaussians_to_raw(g):
    """activated [..., 14] -> raw parameters of the Adam step (and of the .ply): xyz, logit opacity, log scale, quaternion, SH DC."""
    g = g.float()
    o = g[..., 3:4].clamp(1e-6, 1 - 1e-6)
    return torch.cat([g[..., 0:3], torch.log(o / (1 - o)), torch.log(g[..., 4:7].clamp_min(1e-8)), g[..., 7:11],
                      (g[..., 11:14] - 0.5) / SH_C0], dim=-1)


LOSSES = ("mse", "l1_dssim")


def psnr(mse):
    return float("inf") if mse <= 0 else -10.0 * math.log10(mse)


def check_loss(loss, lambda_dssim):
    """ValueError for an unknown loss name or a D-SSIM weight outside [0, 1] (the fitter's and the entrances' common check)."""
    if loss not in LOSSES:
        raise ValueError(f"loss {loss!r}: one of {LOSSES}")
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"lambda_dssim {lambda_dssim}: the D-SSIM weight lies in [0, 1]")


def ssim_workspace(planes, height, width, device):
    """the workspace of vmv_gs_ssim_loss for [planes, height, width] images, as a float tensor"""
    nbytes = C.c_size_t(0)
    L.check(L.load().vmv_gs_ssim_loss_workspace_bytes(planes, height, width, C.byref(nbytes)), "gs_ssim_loss_workspace_bytes")
    return torch.empty((int(nbytes.value) + 3) // 4, dtype=torch.float32, device=device)


def ssim_loss_params(image, target, lambda_dssim, dL, loss, workspace):
    """the argument block of vmv_gs_ssim_loss for contiguous fp32 tensors [..., H, W] (dL: None for the scalars only)"""
    p = L.GsSsimLossParams()
    p.image, p.target = image.data_ptr(), target.data_ptr()
    p.height, p.width = image.shape[-2], image.shape[-1]
    p.planes = image.numel() // (p.height * p.width)
    p.lambda_dssim = float(lambda_dssim)
    p.dL_dimage = dL.data_ptr() if dL is not None else None
    p.loss, p.workspace, p.workspace_bytes = loss.data_ptr(), workspace.data_ptr(), workspace.numel() * 4
    return p


def ssim(image, target):
    """Mean SSIM (11 x 11 Gaussian window, sigma 1.5, zero padding: the 3-D GS / pytorch-ssim definition) of two GPU tensors
    [..., H, W] of equal shape with values in [0, 1]; every [H, W] plane is independent.  The forward of csrc/gs_ssim.hip."""
    if image.shape != target.shape or image.dim() < 2:
        raise ValueError(f"ssim: shapes {tuple(image.shape)} and {tuple(target.shape)}")
    if image.device.type != "cuda" or target.device != image.device:
        raise RuntimeError("ssim runs on the HIP kernel: both images must be on the same GPU")
    a, b = image.detach().to(torch.float32).contiguous(), target.detach().to(torch.float32).contiguous()
    H, W = a.shape[-2], a.shape[-1]
    with torch.cuda.device(a.device):
        ws = ssim_workspace(a.numel() // (H * W), H, W, a.device)
        out = torch.zeros(3, dtype=torch.float32, device=a.device)
        L.check(L.load().vmv_gs_ssim_loss(C.byref(ssim_loss_params(a, b, 1.0, None, out, ws)), _stream_ptr()), "gs_ssim_loss")
        return float(out[2].item())


class GaussianFitter:
    """gaussians [N, 14] or [B, N, 14] (activated), cam_view / cam_view_proj [V, 4, 4] or [B, V, 4, 4], targets [V, 3, S, S] or
    [B, V, 3, S, S] in [0, 1], bg: 3 floats.  ``lr``: dict overriding ``DEFAULT_LR``; ``lr_scale`` multiplies every group.
    ``loss``: "mse" or "l1_dssim" = (1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM)."""

    def __init__(self, gaussians, cam_view, cam_view_proj, targets, bg=(0.5, 0.5, 0.5), lr=None, lr_scale=1.0, fovy=39.6,
                 znear=0.5, zfar=2.5, betas=(0.9, 0.999), eps=1e-15, loss="mse", lambda_dssim=0.2):
        check_loss(loss, lambda_dssim)
        self.loss_name, self.lambda_dssim = loss, float(lambda_dssim)
        g = gaussians if gaussians.dim() == 3 else gaussians.unsqueeze(0)
        cv = cam_view if cam_view.dim() == 4 else cam_view.unsqueeze(0)
        cvp = cam_view_proj if cam_view_proj.dim() == 4 else cam_view_proj.unsqueeze(0)
        tg = targets if targets.dim() == 5 else targets.unsqueeze(0)
        self.device = g.device
        if self.device.type != "cuda":
            raise RuntimeError("GaussianFitter runs on the HIP rasteriser: the Gaussians must be on a GPU")
        self.B, self.N = g.shape[0], g.shape[1]
        self.V, self.S = cv.shape[1], tg.shape[-1]
        if cv.shape[0] != self.B or tuple(tg.shape) != (self.B, self.V, 3, self.S, self.S):
            raise ValueError(f"shapes: gaussians {tuple(g.shape)}, cam_view {tuple(cv.shape)}, targets {tuple(tg.shape)}")
        self.renderer = GaussianRenderer(self.S, fovy, znear, zfar)
        self.bg = [float(v) for v in (bg.reshape(-1)[:3] if torch.is_tensor(bg) else bg)]
        dev = self.device
        self.views = cv.to(dev, torch.float32).reshape(self.B * self.V, 16).contiguous()
        self.view_projs = cvp.to(dev, torch.float32).reshape(self.B * self.V, 16).contiguous()
        self.targets = tg.to(dev, torch.float32).contiguous()
        # scene extent of 3-D GS (cameras_extent): 1.1 x the largest distance of a camera centre from their mean
        centres = torch.inverse(cv.detach().cpu().double().transpose(-1, -2))[..., :3, 3].reshape(-1, 3)
        self.extent = 1.1 * float((centres - centres.mean(0)).norm(dim=1).max()) or 1.0
        lrs = dict(DEFAULT_LR, **(lr or {}))
        self.lr = [lrs["position"] * self.extent * lr_scale, lrs["opacity"] * lr_scale, lrs["scale"] * lr_scale,
                   lrs["rotation"] * lr_scale, lrs["colour"] * lr_scale]
        self.betas, self.eps = betas, eps
        n = self.B * self.N
        self.params = gaussians_to_raw(g.detach()).to(dev).reshape(n, 14).contiguous()
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.gs = torch.empty_like(self.params)
        self.grad = torch.zeros_like(self.params)
        self.t = 0
        VV, S = self.B * self.V, self.S
        self.image = torch.empty(VV, 3, S, S, dtype=torch.float32, device=dev)
        self.alpha = torch.empty(VV, 1, S, S, dtype=torch.float32, device=dev)
        self.final_T = torch.empty(VV, S, S, dtype=torch.float32, device=dev)
        self.n_contrib = torch.empty(VV, S, S, dtype=torch.int32, device=dev)
        self.dL = torch.empty_like(self.image)
        self.grad2d = torch.empty(VV * self.N, 9, dtype=torch.float32, device=dev)
        self.grad_view = torch.empty(VV * self.N, 14, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_ws = torch.empty(1024, dtype=torch.float32, device=dev)
        self.mse = self.loss                           # where _mse() writes
        if loss == "l1_dssim":                         # objective, L1, mean SSIM; the derivative maps and partials of csrc/gs_ssim.hip
            self.loss3 = torch.zeros(3, dtype=torch.float32, device=dev)
            self.loss, self.mse = self.loss3[:1], torch.zeros(1, dtype=torch.float32, device=dev)
            self.ssim_ws = ssim_workspace(VV * 3, S, S, dev)
        self.num_rendered = 0
        self._adam(0)                                  # activated Gaussians of the raw parameters (what the first forward reads)

    # ------------------------------------------------------------------ stages
    def _adam(self, step):
        a = L.GsAdamParams()
        a.params, a.m, a.v, a.grad, a.gaussians = (self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.grad.data_ptr(),
                                                   self.gs.data_ptr())
        a.n, a.step = self.B * self.N, int(step)
        for i, x in enumerate(self.lr):
            a.lr[i] = x
        a.beta1, a.beta2, a.eps = self.betas[0], self.betas[1], self.eps
        L.check(L.load().vmv_gs_adam_step(C.byref(a), _stream_ptr()), "gs_adam_step")

    def _forward(self):
        """Preprocess, size the instance buffers (one host read), forward with state.  -> the backward's argument block."""
        q = L.GsBackwardParams()
        p = q.pass_
        n, ok = self.renderer._batch_setup(p, self.gs, self.views, self.view_projs, self.B, self.V, self.N, self.bg, 1 << 28)
        if not ok:
            raise RuntimeError(f"GaussianFitter: {n} instances — too many for one pass (fewer views or a smaller image)")
        self.num_rendered = n
        p.out_color, p.out_alpha = self.image.data_ptr(), self.alpha.data_ptr()
        q.final_T, q.n_contrib = self.final_T.data_ptr(), self.n_contrib.data_ptr()
        q.dL_dimage, q.grad2d, q.grad_view, q.grad = self.dL.data_ptr(), self.grad2d.data_ptr(), self.grad_view.data_ptr(), self.grad.data_ptr()
        L.check(L.load().vmv_gs_batch_render_state(C.byref(q), _stream_ptr()), "gs_batch_render_state")
        return q

    def _loss(self, with_grad=True):
        """The objective (-> ``loss``) and, ``with_grad``, dL/dimage of the last forward.  l1_dssim: ``loss`` is the first element of
        ``loss3`` = objective, L1, mean SSIM."""
        if self.loss_name == "l1_dssim":
            p = ssim_loss_params(self.image, self.targets, self.lambda_dssim, self.dL if with_grad else None, self.loss3, self.ssim_ws)
            L.check(L.load().vmv_gs_ssim_loss(C.byref(p), _stream_ptr()), "gs_ssim_loss")
            return
        self._mse(with_grad)

    def _mse(self, with_grad):
        L.check(L.load().vmv_gs_image_loss(self.image.data_ptr(), self.targets.data_ptr(), self.image.numel(),
                                           self.dL.data_ptr() if with_grad else None, self.mse.data_ptr(), self.loss_ws.data_ptr(),
                                           _stream_ptr()), "gs_image_loss")

    def _backward(self, q):
        L.check(L.load().vmv_gs_batch_backward(C.byref(q), _stream_ptr()), "gs_batch_backward")

    # ------------------------------------------------------------------ public
    def step(self, events=None):
        """One iteration.  ``events``: optional list that receives CUDA events after each stage (tools/gs_fit_bench.py)."""
        mark = (lambda: events.append(torch.cuda.Event(enable_timing=True)) or events[-1].record()) if events is not None else (lambda: None)
        mark()
        q = self._forward()
        mark()
        self._loss()
        mark()
        L.check(L.load().vmv_gs_batch_backward(C.byref(q), _stream_ptr()), "gs_batch_backward")
        mark()
        self.t += 1
        self._adam(self.t)
        mark()

    def evaluate(self):
        """-> MSE of the current Gaussians against the targets (forward + loss, no update)."""
        self._forward()
        self._mse(False)
        return float(self.mse.item())

    def _evaluate_objective(self):
        """l1_dssim: one forward -> (objective, mean SSIM, MSE) of the same renders."""
        self._forward()
        self._loss(with_grad=False)
        objective, _, s = self.loss3.tolist()
        self._mse(False)
        return objective, s, float(self.mse.item())

    def fit(self, iters):
        """``iters`` iterations -> dict(loss_before, loss_after, psnr_before, psnr_after, ms_per_iter, iters, instances).  ``loss_*`` is
        the optimised objective.  With l1_dssim also mse_before / mse_after (what psnr_* is computed from) and ssim_before /
        ssim_after, the objective's own third scalar."""
        dssim = self.loss_name == "l1_dssim"
        if dssim:
            before, ssim_before, mse_before = self._evaluate_objective()
        else:
            before = mse_before = self.evaluate()
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for _ in range(int(iters)):
            self.step()
        torch.cuda.synchronize(self.device)
        ms = (time.perf_counter() - t0) * 1e3 / max(1, int(iters))
        if dssim:
            after, ssim_after, mse_after = self._evaluate_objective()
        else:
            after = mse_after = self.evaluate()
        st = dict(loss_before=before, loss_after=after, psnr_before=psnr(mse_before), psnr_after=psnr(mse_after), ms_per_iter=ms,
                  iters=int(iters), instances=self.num_rendered)
        if dssim:
            st.update(mse_before=mse_before, mse_after=mse_after, ssim_before=ssim_before, ssim_after=ssim_after)
        return st

    def gaussians(self):
        """activated Gaussians [N, 14] (or [B, N, 14] for B > 1), a copy"""
        g = self.gs.detach().clone().reshape(self.B, self.N, 14)
        return g[0] if self.B == 1 else g

    def images(self):
        """the last forward's renders [B, V, 3, S, S]"""
        return self.image.reshape(self.B, self.V, 3, self.S, self.S)
