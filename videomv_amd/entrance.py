"""``inference_text2video_entrance`` — the INFER_ENGINE plugin of ``inference.py --cfg configs/t2v_infer.yaml``
(tools/inferences/inference_text2video_entrance.py:37-328) over the HIP hot path.

Kept: config layering (python defaults <- YAML/CLI dict-merge <- ``vldm_cfg`` overlay), one process per GPU with
``seed + rank`` (replicas), registry-built DIFFUSION / EMBEDDER / AUTO_ENCODER / MODEL, checkpoint formats
(``state_dict``/``step`` wrapper, ``strict=False``), orbit ``camera_data``, latent noise shape
``[1, 4, max_frames, res_y/scale, res_x/scale]``, CFG kwargs pair, 50-step DDIM (``cfg.ddim_timesteps``, new key — the
reference hard-codes 50 at :264), VAE decode in ``decoder_bs`` chunks, output naming.
Different by design: launches go to ``libvmv_hip_{f16,bf16}.so`` (``hip_dtype`` config key / ``VMV_DTYPE``); per sample the entrance
writes the reference's frame PNGs (``<name>/{fid:05d}.png``) and ``<name>.mp4`` when an H.264 encoder exists (none ships here),
plus a ``.pt`` tensor and a PNG contact sheet; the second, LGM-refined loop (:271-278)
runs when ``UNet.use_lgm_refine`` is set (also under ``frame_parallel``; not under ``cfg_parallel``).
"""
import logging
import os
import os.path as osp
import re
import sys

import torch
import torch.distributed as dist

from .config import default_cfg, merge_into, assign_signle_cfg, AttrDict
from .registry import INFER_ENGINE, MODEL, EMBEDDER, AUTO_ENCODER, DIFFUSION
from .camera import entrance_camera_data
from .pipeline import sample_views
from .dist import rank_seed, shard_prompts
from . import embedder as _embedder  # noqa: F401  (registers the embedders)
from . import gs_export
from .video_io import _save_contact_sheet, _save_frames_safe, save_video_frames  # noqa: F401  (save_video_frames: the writer's public name)


def _plain(d):
    return {k: (_plain(v) if isinstance(v, dict) else v) for k, v in d.items()}


def _load_weights(module, path, allow_random, what, prefix_filter=None):
    if path and osp.exists(path):
        sd = torch.load(path, map_location="cpu")
        if "state_dict" in sd:
            sd = sd["state_dict"]
        if prefix_filter:
            sd = {k.split(prefix_filter)[-1]: v for k, v in sd.items() if prefix_filter in k}
        status = module.load_state_dict(sd, strict=False)
        logging.info(f"Load {what} from {path} with status {status}")
        return True
    if not allow_random:
        raise FileNotFoundError(f"{what} checkpoint {path!r} not found (set allow_random_init True to run on "
                                f"random weights)")
    logging.warning(f"{what}: checkpoint {path!r} missing -> RANDOM weights (allow_random_init)")
    g = torch.Generator().manual_seed(1234)
    for name, p in module.named_parameters():
        if p.dim() > 1:
            p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5))
        elif name.endswith("bias"):
            p.zero_()
        else:
            p.fill_(1.0)
    return False


@INFER_ENGINE.register_function()
def inference_text2video_entrance(cfg_update, **kwargs):
    cfg = default_cfg()
    merge_into(cfg, _plain(dict(cfg_update)))
    cfg.pmi_rank = int(os.getenv('RANK', 0))
    cfg.pmi_world_size = int(os.getenv('WORLD_SIZE', 1))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29533')
    cfg.world_size = 1 if cfg.debug else cfg.pmi_world_size       # launched one rank per GPU by torch.distributed.run
    return worker(int(os.getenv('LOCAL_RANK', 0)), cfg, cfg_update)   # (returns the worker's merged cfg)


def _warn_bf16(name):
    """bf16 is the range fallback, not a parity configuration (configs/*.yaml): say so once, where the user chose it."""
    if str(name).lower() in ("bf16", "bfloat16"):
        import warnings
        warnings.warn("hip_dtype: bf16 — the wide-range build; measured 1.3e-2 rel-L2 per UNet forward against the fp32 reference, outside "
                      "the 1e-2 parity tolerance that the default fp16 build meets (use it only for checkpoints that overflow fp16)")


@torch.no_grad()
def worker(gpu, cfg, cfg_update):
    if 'vldm_cfg' in cfg_update and cfg_update['vldm_cfg']:
        cfg = AttrDict(assign_signle_cfg(cfg, cfg_update, 'vldm_cfg'))
        merge_into(cfg, _plain(dict(cfg_update)))
    cfg.gpu, cfg.seed = gpu, int(cfg.seed)
    if cfg.get('hip_dtype'):                        # (not a reference key) 16-bit storage type of the kernels: fp16 | bf16
        from . import _lib
        _lib.set_elem(cfg.hip_dtype)
        _warn_bf16(cfg.hip_dtype)
    cfg.rank = cfg.pmi_rank
    # frame_parallel (not a reference key; BASELINE configs[2]): the ranks share ONE sample — same seed, F / N views each
    fpar = bool(cfg.get('frame_parallel', False)) and cfg.world_size > 1
    gs_export._check_export_cfg(cfg, bool(dict(cfg.UNet).get('use_lgm_refine')) and not (fpar and bool(cfg.get('cfg_parallel', False))))
    torch.manual_seed(cfg.seed if fpar else rank_seed(cfg.seed, cfg.rank))
    on_gpu = str(cfg.device).startswith("cuda")
    device = torch.device("cuda", gpu) if on_gpu else torch.device(cfg.device)
    if on_gpu:
        torch.cuda.set_device(gpu)
    if cfg.world_size > 1:
        dist.init_process_group(backend='nccl' if on_gpu else 'gloo', world_size=cfg.world_size, rank=cfg.rank)

    exp_name = osp.basename(cfg.test_list_path).split('.')[0]
    cfg.log_dir = osp.join(cfg.log_dir, exp_name)
    os.makedirs(cfg.log_dir, exist_ok=True)
    logging.basicConfig(level=logging.INFO, format='[%(asctime)s] %(levelname)s: %(message)s', force=True,
                        handlers=[logging.FileHandler(osp.join(cfg.log_dir, 'log_%02d.txt' % cfg.rank)),
                                  logging.StreamHandler(stream=sys.stdout)])
    logging.info(f"Going into inference_text2video_entrance inference on {gpu} gpu (HIP hot path)")

    diffusion = DIFFUSION.build(dict(cfg.Diffusion))
    clip_encoder = EMBEDDER.build(dict(cfg.embedder))
    _, _, zero_y_negative = clip_encoder(text=[""])
    autoencoder = AUTO_ENCODER.build({k: v for k, v in cfg.auto_encoder.items() if k != 'pretrained'})
    _load_weights(autoencoder, cfg.auto_encoder.get('pretrained'), cfg.allow_random_init, "autoencoder",
                  prefix_filter='first_stage_model.')
    autoencoder.eval()
    unet_cfg = dict(cfg.UNet)
    # (LGM-refined steps run frame-parallel too since round 4 — every rank renders / re-encodes its own views; not with cfg_parallel)
    use_lgm = bool(unet_cfg.get('use_lgm_refine')) and not (fpar and bool(cfg.get('cfg_parallel', False)))
    unet_cfg['use_lgm_refine'] = use_lgm
    if use_lgm and cfg.get('lgm_opt'):              # (not a reference key: shrinks the LGM for CPU plumbing tests)
        unet_cfg['lgm_opt'] = _plain(dict(cfg.lgm_opt))
    model = MODEL.build(unet_cfg)
    _load_weights(model, cfg.get('test_model'), cfg.allow_random_init, "UNet")
    model.eval()
    if fpar:
        from .comm import FrameComm, CfgFrameComm
        # cfg_parallel (not a reference key): 2 x N/2 — one CFG branch per half of the ranks, frames sharded inside each half
        model.set_frame_parallel(CfgFrameComm() if bool(cfg.get('cfg_parallel', False)) else FrameComm())
        logging.info(f"frame-parallel sampling: {cfg.world_size} ranks x {int(cfg.num_views or cfg.max_frames) // cfg.world_size} views")

    with open(cfg.test_list_path, 'r') as f:
        test_list = [ln.strip() for ln in f.readlines()]
    # `shard_prompts: True` (not a reference key): rank r takes prompts r, r + W, ... instead of every rank running the whole list
    # with seed + rank (the reference's behaviour, :152-156, and the default)
    if not fpar:
        test_list = shard_prompts(test_list, cfg.rank, max(1, int(cfg.get('world_size', 1))), replicate=not cfg.get('shard_prompts', False))
    F = int(cfg.num_views or cfg.max_frames)
    lat_h, lat_w = int(cfg.resolution[1] / cfg.scale), int(cfg.resolution[0] / cfg.scale)
    outputs = []
    # `prompt_batch: b` (not a reference key; default 1 = the reference's one prompt at a time, :152-214): b prompts are denoised in ONE
    # plan per step (noise [b, 4, F, h, w], y [b, 77, 1024] — the shapes the reference's sampler API admits, diffusion_ddim.py:247-260).
    # One sample's small levels do not fill 256 CUs: 2 prompts per plan = +22 % samples/s at 256 px, +6 % at 320 x 512.
    # Noises are drawn per prompt in list order, so every sample starts from the noise the unbatched run gives it (without the LGM-refined
    # loop; with it the refined steps' posterior draws sit between two prompts' noises in the unbatched run, so the noises — not their
    # distribution — differ).  The LGM-refined second loop is batched too: its 47 plain steps in one plan, the 3 refined ones sample by
    # sample (diffusion_ddim.ddim_sample_loop).  Over a frame-parallel group (plain `frame_parallel`, no LGM loop) every rank denoises its
    # frames of all b prompts in one plan.
    # (the fused LGM steps are GPU-only; over a frame-parallel group: plain FrameComm without the LGM loop — DESIGN 8)
    one_only = (use_lgm and (not on_gpu or fpar)) or (fpar and bool(cfg.get('cfg_parallel', False)))
    pbatch = 1 if one_only else max(1, int(cfg.get('prompt_batch', 1) or 1))
    elevation, camera_dist = 15, 2.0
    gs_exports = []

    def run_group(group):
        camera_data = entrance_camera_data(F, elevation=elevation, camera_distance=camera_dist)
        ys = [clip_encoder(text=[cap])[2] for _, cap in group]
        noises = [torch.randn([1, 4, F, lat_h, lat_w]) for _ in group]
        y_words, noise = torch.cat(ys, dim=0), torch.cat(noises, dim=0).to(device)
        y_neg = zero_y_negative.to(device).expand(len(group), -1, -1).contiguous()      # (the reference's forward wants y of the noise's batch)
        x0_all, video_all = sample_views(model, diffusion, autoencoder, noise, y_words.to(device), y_neg,
                                         camera_data, guide_scale=cfg.guide_scale, ddim_timesteps=int(cfg.ddim_timesteps),
                                         decoder_bs=int(cfg.decoder_bs), scale_factor=cfg.scale_factor)
        x0_gs_all = video_gs_all = None
        if use_lgm:       # second, LGM-refined loop from the SAME noise (inference_text2video_entrance.py:267-279,302-311)
            from .lgm import prepare_gs_data
            from .pipeline import decode_views
            gs_data = prepare_gs_data(camera_data, model.lgm_opt)
            kw = [dict(y=y_words.to(device), camera_data=camera_data, gs_data=gs_data),
                  dict(y=y_neg, camera_data=camera_data, gs_data=gs_data)]
            x0_gs_all = diffusion.ddim_sample_loop(noise=noise, model=model, autoencoder=autoencoder, model_kwargs=kw,
                                                   guide_scale=cfg.guide_scale, ddim_timesteps=int(cfg.ddim_timesteps), eta=0.0)
            video_gs_all = decode_views(autoencoder, x0_gs_all, int(cfg.decoder_bs), cfg.scale_factor)
        if fpar and cfg.rank != 0:          # every rank holds the gathered views; rank 0 writes them
            return
        export = lambda video_gs, path: gs_export._export_gaussians(cfg, model, video_gs, camera_data, gs_data, elevation, camera_dist, path, device)
        for s, (idx, caption) in enumerate(group):
            cap_name = re.sub(r'[^\w\s]', '', caption).replace(' ', '_')
            name = f'{idx:04d}_{cap_name}_{int(elevation):02d}_{camera_dist:.02f}'
            _write_sample(cfg, name, {'caption': caption}, s, (x0_all, video_all), (x0_gs_all, video_gs_all), export, outputs, gs_exports)

    pending = []
    for idx, caption in enumerate(test_list):
        if caption.startswith('#') or caption == "":
            logging.info(f'Skip {caption!r}')
            continue
        if '3d asset' not in caption:
            caption = caption + ", 3d asset"
        logging.info(f"[{idx}]/[{len(test_list)}] Begin to sample {caption} ...")
        pending.append((idx, caption))
        if len(pending) == pbatch:
            run_group(pending)
            pending = []
    if pending:
        run_group(pending)
    return _finish(cfg, model, on_gpu, outputs, gs_exports)


def _write_sample(cfg, name, source, s, plain, refined, export, outputs, gs_exports):
    """Sample ``s`` of a group's (latents, videos) ``plain``: ``<stem>.pt`` (with ``source``: the caption or the image's path), the sheet, the
    reference's <stem>.mp4 + frame PNGs; the same as ``<stem>_gs`` for ``refined`` (the LGM-refined loop: the reference's second file),
    and with ``save_gaussians`` their 3-D asset, ``export(video_gs, stem)``."""
    stem = osp.join(cfg.log_dir, f'rank_{cfg.world_size:02d}_{cfg.rank:02d}_{name}')
    for tag, (x0, video) in (('', plain), ('_gs', refined)):
        if video is None:
            continue
        x0, video = x0[s:s + 1], video[s:s + 1]
        torch.save({'latent': x0.cpu(), 'video': video.cpu(), **source}, stem + tag + '.pt')
        _save_contact_sheet(video.cpu(), stem + tag + '.png', cfg.mean, cfg.std)
        _save_frames_safe(stem + tag + '.mp4', video, cfg)
        if tag and cfg.get('save_gaussians'):
            gs_exports.append(export(video, stem))
    logging.info('Save views to %s' % (stem + '.pt'))
    outputs.append(stem + '.pt')


def _finish(cfg, model, on_gpu, outputs, gs_exports):
    """The end of both workers: wait for the device, close the process group, hand the written paths over in ``cfg``."""
    logging.info('Congratulations! The inference is completed!')
    if on_gpu:
        torch.cuda.synchronize()
    if cfg.world_size > 1:
        fc = getattr(getattr(model, "module", model), "frame_comm", None)
        if fc is not None and hasattr(fc, "close"):
            fc.close()              # the native RCCL communicators (and twins) go first: collective, every rank gets here
        dist.barrier()
        dist.destroy_process_group()
    cfg.outputs = outputs
    if cfg.get('save_gaussians'):
        cfg.gs_exports = gs_exports
    return cfg


def center_crop_wide(img, size):
    """utils/transforms.py:163-183 — BOX-resize so that the image covers ``size`` (w, h), then centre-crop."""
    from PIL import Image
    scale = min(img.size[0] / size[0], img.size[1] / size[1])
    img = img.resize((round(img.width // scale), round(img.height // scale)), resample=Image.BOX)
    x1, y1 = (img.width - size[0]) // 2, (img.height - size[1]) // 2
    return img.crop((x1, y1, x1 + size[0], y1 + size[1]))


def _to_normalised_tensor(img, mean, std):
    import numpy as np
    a = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
    return (a - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)


@INFER_ENGINE.register_function()
def inference_i2vgen_entrance(cfg_update, **kwargs):
    """Image -> 24 views (tools/inferences/inference_i2vgen_entrance.py): RGBA image on a white background -> VAE-encoded
    ``local_image`` + CLIP image feature -> UNetSD_I2VGen with v-prediction / cosine-ZTSNR DDIM, guide 6, orbit cameras
    at elevation 5 / distance 1.7 (:136-147), fps 8; decode in ``decoder_bs`` chunks."""
    cfg = default_cfg()
    cfg.negative_prompt = 'Distorted, discontinuous, Ugly, blurry, low resolution, motionless, static, disfigured, ' \
                          'disconnected limbs, Ugly faces, incomplete arms'
    merge_into(cfg, _plain(dict(cfg_update)))
    cfg.pmi_rank, cfg.pmi_world_size = int(os.getenv('RANK', 0)), int(os.getenv('WORLD_SIZE', 1))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29534')
    cfg.world_size = 1 if cfg.debug else cfg.pmi_world_size
    return worker_i2v(int(os.getenv('LOCAL_RANK', 0)), cfg, cfg_update)


@torch.no_grad()
def worker_i2v(gpu, cfg, cfg_update):
    from PIL import Image
    if 'vldm_cfg' in cfg_update and cfg_update['vldm_cfg']:
        cfg = AttrDict(assign_signle_cfg(cfg, cfg_update, 'vldm_cfg'))
        merge_into(cfg, _plain(dict(cfg_update)))
    cfg.gpu, cfg.seed, cfg.rank = gpu, int(cfg.seed), cfg.pmi_rank
    gs_export._check_export_cfg(cfg, bool(dict(cfg.UNet).get('use_lgm_refine')))
    if cfg.get('hip_dtype'):                        # (not a reference key) 16-bit storage type of the kernels: fp16 | bf16
        from . import _lib
        _lib.set_elem(cfg.hip_dtype)
        _warn_bf16(cfg.hip_dtype)
    torch.manual_seed(rank_seed(cfg.seed, cfg.rank))
    on_gpu = str(cfg.device).startswith("cuda")
    device = torch.device("cuda", gpu) if on_gpu else torch.device(cfg.device)
    if on_gpu:
        torch.cuda.set_device(gpu)
    if cfg.world_size > 1:
        dist.init_process_group(backend='nccl' if on_gpu else 'gloo', world_size=cfg.world_size, rank=cfg.rank)
    exp_name = osp.basename(cfg.test_list_path).split('.')[0]
    cfg.log_dir = osp.join(cfg.log_dir, exp_name)
    os.makedirs(cfg.log_dir, exist_ok=True)
    logging.basicConfig(level=logging.INFO, format='[%(asctime)s] %(levelname)s: %(message)s', force=True,
                        handlers=[logging.FileHandler(osp.join(cfg.log_dir, 'log_%02d.txt' % cfg.rank)),
                                  logging.StreamHandler(stream=sys.stdout)])
    logging.info(f"Going into inference_i2vgen_entrance inference on {gpu} gpu (HIP hot path)")
    diffusion = DIFFUSION.build(dict(cfg.Diffusion))
    clip_encoder = EMBEDDER.build(dict(cfg.embedder))
    _, _, zero_y_negative = clip_encoder(text=cfg.negative_prompt)
    black_image_feature = torch.zeros([1, 1, cfg.UNet['y_dim']])
    autoencoder = AUTO_ENCODER.build({k: v for k, v in cfg.auto_encoder.items() if k != 'pretrained'})
    _load_weights(autoencoder, cfg.auto_encoder.get('pretrained'), cfg.allow_random_init, "autoencoder",
                  prefix_filter='first_stage_model.')
    autoencoder.eval()
    unet_cfg = dict(cfg.UNet)
    use_lgm = bool(unet_cfg.get('use_lgm_refine'))
    if use_lgm and cfg.get('lgm_opt'):              # (not a reference key: shrinks the LGM for CPU plumbing tests)
        unet_cfg['lgm_opt'] = _plain(dict(cfg.lgm_opt))
    model = MODEL.build(unet_cfg)
    _load_weights(model, cfg.get('test_model'), cfg.allow_random_init, "UNet")
    model.eval()
    F = int(cfg.num_views or cfg.max_frames)
    elevation, camera_dist = 5, 1.7
    camera_data = entrance_camera_data(F, elevation=elevation, camera_distance=camera_dist)
    with open(cfg.test_list_path, 'r') as f:
        test_list = [ln.strip() for ln in f.readlines() for _ in range(int(cfg.get('round', 1)))]
    lat_h, lat_w = int(cfg.resolution[1] / cfg.scale), int(cfg.resolution[0] / cfg.scale)
    outputs = []
    # `prompt_batch: b` (not a reference key; default 1 = the reference's one image at a time, inference_i2vgen_entrance.py:215-300): b input
    # images are denoised in ONE plan per step (unet_i2vgen._forward_cfg_rows_batched): +23 % samples/s at 256 px, +7 % at 320 x 512 with
    # b = 2.  Noises are drawn per image in list order; the LGM-refined second loop is batched too (47 plain steps in one plan, the 3
    # refined ones sample by sample: diffusion_ddim.ddim_sample_loop).
    pbatch = 1 if (use_lgm and not on_gpu) else max(1, int(cfg.get('prompt_batch', 1) or 1))
    gs_exports = []

    def run_group(group):
        ys, vis, locs, noises = [], [], [], []
        for idx, line, image in group:
            vit_img = center_crop_wide(image, (cfg.resolution[0], cfg.resolution[0])).resize(tuple(cfg.get('vit_resolution', [224, 224])))
            y_visual, _, y_words = clip_encoder(image=_to_normalised_tensor(vit_img, cfg.mean, cfg.std).unsqueeze(0), text=[""])
            img_t = _to_normalised_tensor(center_crop_wide(image, tuple(cfg.resolution)), cfg.mean, cfg.std).unsqueeze(0).to(device)
            local_image = autoencoder.encode_firsr_stage(img_t, cfg.scale_factor)
            ys.append(y_words.to(device)); vis.append(y_visual.unsqueeze(1).to(device))
            locs.append(local_image.unsqueeze(2).repeat_interleave(repeats=F, dim=2))
            noises.append(torch.randn([1, 4, F, lat_h, lat_w]))
        n = len(group)
        y_words, y_visual, local_image = torch.cat(ys, dim=0), torch.cat(vis, dim=0), torch.cat(locs, dim=0)
        noise = torch.cat(noises, dim=0).to(device)
        fps_tensor = torch.tensor([cfg.target_fps], dtype=torch.long, device=device)
        infer_img = black_image_feature if cfg.use_zero_infer else None
        rep = lambda v: v.to(device).expand(n, *v.shape[1:]).contiguous()        # (the reference's forward wants kwargs of the noise's batch)
        kw = [{'y': y_words, 'image': y_visual, 'local_image': local_image, 'fps': fps_tensor, 'camera_data': camera_data},
              {'y': rep(zero_y_negative), 'image': None if infer_img is None else rep(infer_img),
               'local_image': local_image, 'fps': fps_tensor, 'camera_data': camera_data}]
        x0_all = diffusion.ddim_sample_loop(noise=noise, model=model, model_kwargs=kw, guide_scale=cfg.guide_scale,
                                            ddim_timesteps=int(cfg.ddim_timesteps), eta=0.0)
        from .pipeline import decode_views
        video_all = decode_views(autoencoder, x0_all, int(cfg.decoder_bs), cfg.scale_factor)
        x0_gs_all = video_gs_all = gs_data = None
        if use_lgm:       # second, LGM-refined loop from the same noise (inference_i2vgen_entrance.py:281-292)
            from .lgm import prepare_gs_data
            gs_data = prepare_gs_data(camera_data, model.lgm_opt)
            kw_gs = [dict(k, gs_data=gs_data) for k in kw]
            x0_gs_all = diffusion.ddim_sample_loop(noise=noise, model=model, autoencoder=autoencoder, model_kwargs=kw_gs,
                                                   guide_scale=cfg.guide_scale, ddim_timesteps=int(cfg.ddim_timesteps), eta=0.0)
            video_gs_all = decode_views(autoencoder, x0_gs_all, int(cfg.decoder_bs), cfg.scale_factor)
        export = lambda video_gs, path: gs_export._export_gaussians(cfg, model, video_gs, camera_data, gs_data, elevation, camera_dist, path, device)
        for s_, (idx, line, _) in enumerate(group):
            name = f'{idx:04d}_{osp.basename(line).split(".")[0]}_{int(elevation):02d}_{camera_dist:.02f}'
            _write_sample(cfg, name, {'image': line}, s_, (x0_all, video_all), (x0_gs_all, video_gs_all), export, outputs, gs_exports)

    pending = []
    for idx, line in enumerate(test_list):
        if line.startswith('#') or line == "":
            logging.info(f'Skip {line!r}')
            continue
        try:
            rgba = Image.open(line).convert('RGBA')
        except Exception as e:
            logging.info(f'cannot open {line}: {e}')
            continue
        logging.info(f"[{idx}]/[{len(test_list)}] Begin to sample {line} ...")
        image = Image.new('RGB', size=rgba.size, color=(255, 255, 255))
        image.paste(rgba, (0, 0), mask=rgba)
        pending.append((idx, line, image))
        if len(pending) == pbatch:
            run_group(pending)
            pending = []
    if pending:
        run_group(pending)
    return _finish(cfg, model, on_gpu, outputs, gs_exports)
