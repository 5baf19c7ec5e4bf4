"""The 3-D asset export of the entrances (``save_gaussians`` and the ``gs_*`` keys, none a reference key): ONE table of the
settings' defaults and validators, the check that refuses a bad combination before any sampling, and one function per stage under the
driver ``_export_gaussians``.  No RNG.  ``gs``, ``gs_fit``, ``gs_mesh`` and ``lgm`` are reached through their modules at call time."""
import collections
import itertools
import logging
import math
from types import SimpleNamespace

import torch

from . import gs, gs_fit, gs_mesh, lgm
from .video_io import _save_contact_sheet, _save_frames_safe


def _is_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


_POSITIVE = (lambda v: float(v) > 0, "{k} must be positive, got {v}")
# key -> default (config.py documents the keys), validator of a value that is set, its refusal, whether 0 / '' read as "not set"
_Setting = collections.namedtuple("_Setting", "default valid message zero_unset", defaults=(None, None, False))
SETTINGS = {
    "gs_fit_iters": _Setting(0),
    "gs_fit_loss": _Setting("mse", zero_unset=True),
    "gs_fit_lambda_dssim": _Setting(0.2),
    "gs_fit_lr_scale": _Setting(1.0, zero_unset=True),
    "gs_orbit_views": _Setting(0),
    "gs_orbit_elevation": _Setting(None),
    "gs_orbit_size": _Setting(None, zero_unset=True),
    "gs_points_voxel": _Setting(None, *_POSITIVE),
    "gs_mesh_res": _Setting(128, lambda v: 16 <= int(v) <= 512, "{k} must be in [16, 512], got {v}", zero_unset=True),
    "gs_mesh_extent": _Setting(None, *_POSITIVE),
    "gs_mesh_trunc": _Setting(None, *_POSITIVE),
    "gs_mesh_min_component": _Setting(None, lambda v: _is_number(v) and 0.0 <= float(v) <= 1.0,
                                      "{k} must be a fraction in [0, 1] of the largest component's faces, got {v!r}"),
    "gs_mesh_elevations": _Setting(None, lambda v: isinstance(v, (list, tuple)) and all(
        _is_number(e) and math.isfinite(float(e)) and -90.0 < float(e) < 90.0 for e in v),
        "{k} must be a list of elevations in degrees inside (-90, 90), got {v!r}"),
    "gs_mesh_texture_patch": _Setting(8, lambda v: isinstance(v, int) and not isinstance(v, bool) and 4 <= v <= 32,
                                      "{k} must be a whole number of texels in [4, 32], got {v!r}"),
}


def _setting(cfg, key, check=False):
    """cfg[key], or the table's default where the key is not set; with ``check`` a value other than None must pass the table's validator"""
    v, s = cfg.get(key), SETTINGS[key]
    v = s.default if v is None or (s.zero_unset and not v) else v
    if check and v is not None and not s.valid(v):
        raise ValueError(s.message.format(k=key, v=v))
    return v


def _check_export_cfg(cfg, use_lgm):
    """`save_gaussians` exports the LGM-refined loop's Gaussians: refuse it, before any sampling, where that loop does not run or cannot
    run (the LGM renders square views only), or where the fit's objective is not one the fitter knows."""
    geometry = [k for k in ('gs_orbit_depth', 'gs_points', 'gs_points_voxel', 'gs_mesh') if cfg.get(k)]
    if geometry and not (cfg.get('save_gaussians') and int(_setting(cfg, 'gs_orbit_views')) > 0):
        raise ValueError(f"{' / '.join(geometry)}: depth maps, the point cloud and the mesh come from the orbit render of the exported "
                         "Gaussians: set save_gaussians True and gs_orbit_views > 0")
    if cfg.get('gs_points_voxel') and not cfg.get('gs_points'):
        raise ValueError("gs_points_voxel is the voxel size of the gs_points export: set gs_points True")
    if cfg.get('gs_points'):
        _setting(cfg, 'gs_points_voxel', check=True)
    if not cfg.get('gs_mesh'):
        sub = [k for k in ('gs_mesh_extent', 'gs_mesh_trunc', 'gs_mesh_min_component', 'gs_mesh_elevations') if cfg.get(k) is not None]
        sub += ['gs_mesh_res'] if int(_setting(cfg, 'gs_mesh_res')) != SETTINGS['gs_mesh_res'].default else []
        sub += ['gs_mesh_texture'] if cfg.get('gs_mesh_texture') else []
        sub += ['gs_mesh_texture_patch'] if _setting(cfg, 'gs_mesh_texture_patch') != SETTINGS['gs_mesh_texture_patch'].default else []
        if sub:
            raise ValueError(f"{' / '.join(sub)}: a setting of the gs_mesh export: set gs_mesh True")
    else:
        for k in ('gs_mesh_res', 'gs_mesh_extent', 'gs_mesh_trunc', 'gs_mesh_min_component', 'gs_mesh_elevations', 'gs_mesh_texture_patch'):
            _setting(cfg, k, check=True)
    if not cfg.get('save_gaussians'):
        return
    if not use_lgm:
        raise ValueError("save_gaussians needs the LGM-refined loop: set UNet.use_lgm_refine True (and no cfg_parallel)")
    if int(cfg.resolution[0]) != int(cfg.resolution[1]):
        raise ValueError(f"save_gaussians: the LGM branch renders square views, resolution {list(cfg.resolution)} is not square")
    try:
        gs_fit.check_loss(*_fit_loss(cfg))
    except ValueError as e:
        raise ValueError(f"save_gaussians: gs_fit_loss / gs_fit_lambda_dssim: {e}") from None


def _fit_loss(cfg):                                                     # -> (gs_fit_loss, gs_fit_lambda_dssim)
    return str(_setting(cfg, 'gs_fit_loss')), float(_setting(cfg, 'gs_fit_lambda_dssim'))


@torch.no_grad()
def _export_gaussians(cfg, model, video_gs, camera_data, gs_data, elevation, camera_dist, stem, device):
    """The 3-D asset of one LGM-refined sample: the LGM on its final key views (LgmRefiner.gaussians_from_views) as ``<stem>_gs.ply``, then
    the stages below as the keys ask.  No RNG (the next prompt's noise stays the same).  -> dict of paths and statistics (cfg.gs_exports)."""
    refiner = model.lgm_refiner(device)
    F_ = video_gs.shape[2]
    idxs = [0, 6, 12, 18] if F_ == 24 else [i * F_ // 4 for i in range(4)]
    views = video_gs[0].permute(1, 0, 2, 3).to(device, torch.float32)                 # [F, 3, H, W] in [-1, 1]
    g = refiner.gaussians_from_views(views[idxs].contiguous(), gs_data)              # [1, N, 14]
    rec = dict(ply=stem + '_gs.ply', fit_iters=int(_setting(cfg, 'gs_fit_iters')))
    if rec['fit_iters'] > 0:
        g = _fit(cfg, refiner, g, views, gs_data, rec)
    rec['vertices'] = refiner.renderer.save_ply(g, rec['ply'])
    logging.info(f"Save 3D Gaussians ({rec['vertices']} of {g.shape[1]}) to {rec['ply']}")
    n_orbit = int(_setting(cfg, 'gs_orbit_views'))
    if n_orbit > 0:
        elev = _setting(cfg, 'gs_orbit_elevation')
        o = _render_orbit(cfg, refiner, g.to(device), camera_data, n_orbit, elevation if elev is None else float(elev), camera_dist, stem, rec)
        if cfg.get('gs_orbit_depth'):
            rec['orbit_depth'], rec['orbit_depth_sheet'] = stem + '_gs_orbit_depth.npy', stem + '_gs_orbit_depth.png'
            _save_depth_maps(o.out["median_depth"][0, :, 0].float().cpu(), rec['orbit_depth'], rec['orbit_depth_sheet'], o.opt.znear, o.opt.zfar)
            logging.info(f"Save {n_orbit} median-depth maps to {rec['orbit_depth']}")
        if cfg.get('gs_points'):
            _export_points(cfg, o, stem, rec)
        if cfg.get('gs_mesh'):
            mesh = _write_mesh(cfg, o, stem, rec)
            if cfg.get('gs_mesh_texture'):
                _write_texture(cfg, o, stem, rec, *mesh)
    return rec


def _fit(cfg, refiner, g, views, gs_data, rec):
    """Fit the Gaussians to all decoded views (gs_fit.GaussianFitter: targets video * 0.5 + 0.5 against the refiner's background)"""
    opt, (loss, lam) = refiner.opt, _fit_loss(cfg)
    fitter = gs_fit.GaussianFitter(g[0], gs_data['cam_view'][0], gs_data['cam_view_proj'][0], (views * 0.5 + 0.5).contiguous(),
                                   bg=(refiner.bg_color,) * 3, lr_scale=float(_setting(cfg, 'gs_fit_lr_scale')), fovy=opt.fovy, znear=opt.znear,
                                   zfar=opt.zfar, loss=loss, lambda_dssim=lam)
    st = fitter.fit(rec['fit_iters'])
    rec.update(st)
    logging.info(f"gs fit: {rec['fit_iters']} iterations on {views.shape[0]} views, PSNR {st['psnr_before']:.2f} -> {st['psnr_after']:.2f} dB "
                 f"(loss {st['loss_before']:.3e} -> {st['loss_after']:.3e})"
                 + (f", SSIM {st['ssim_before']:.4f} -> {st['ssim_after']:.4f}" if 'ssim_after' in st else "")
                 + f", {st['ms_per_iter']:.2f} ms/iteration, {st['instances']} instances")
    return fitter.gaussians().unsqueeze(0)


def _orbit(o, elevation, depth):
    """One orbit of ``o.n`` cameras at ``elevation`` -> (its render, in the rasteriser's depth mode if ``depth``; its cameras [1, n, 4, 4])"""
    cv, cvp = lgm.orbit_cameras(o.camera_data, o.n, elevation, o.camera_dist, o.opt)
    return (o.renderer.render_depth if depth else o.renderer.render)(o.g, cv.to(o.dev), cvp.to(o.dev), None, bg_color=o.bgc), cv


def _render_orbit(cfg, refiner, g, camera_data, n_orbit, elev, camera_dist, stem, rec):
    """Render the orbit ONCE, in depth mode only if a geometry export wants it; write its sheet and frames.  -> what the stages share"""
    opt = refiner.opt
    o = SimpleNamespace(g=g, dev=g.device, camera_data=camera_data, camera_dist=camera_dist, n=n_orbit, opt=opt, bg=refiner.bg_color,
                        bgc=torch.full((3,), refiner.bg_color, dtype=torch.float32, device=g.device),
                        renderer=gs.GaussianRenderer(int(_setting(cfg, 'gs_orbit_size') or opt.output_size), opt.fovy, opt.znear, opt.zfar))
    o.out, o.cv = _orbit(o, elev, bool(cfg.get('gs_orbit_depth') or cfg.get('gs_points') or cfg.get('gs_mesh')))
    mean, std = torch.tensor(cfg.mean).view(1, 3, 1, 1, 1), torch.tensor(cfg.std).view(1, 3, 1, 1, 1)
    video = (o.out["image"].float().cpu().permute(0, 2, 1, 3, 4) - mean) / std          # [1, 3, n, S, S], the entrance's range
    rec['orbit_sheet'], rec['orbit_frames'] = stem + '_gs_orbit.png', stem + '_gs_orbit'
    _save_contact_sheet(video, rec['orbit_sheet'], cfg.mean, cfg.std)
    _save_frames_safe(stem + '_gs_orbit.mp4', video, cfg)
    return o


def _camera_distance(o):
    """the distance of the first orbit camera from the origin of the Gaussians' frame"""
    return float(torch.inverse(o.cv[0, 0].float().cpu())[3, :3].norm())


def _write_mesh(cfg, o, stem, rec):
    """``_gs_mesh.ply``: TSDF fusion of the orbit and of one more per ``gs_mesh_elevations`` entry (rendered for the fusion alone), surface
    nets, small components dropped.  -> verts, colours, faces, with gs_mesh_texture [(depth, colour, cameras) per fused orbit], the voxel size"""
    res, half, trunc = int(_setting(cfg, 'gs_mesh_res')), _setting(cfg, 'gs_mesh_extent'), _setting(cfg, 'gs_mesh_trunc')
    # default cube: the ball every orbit view sees whole, d sin(fovy / 2) around the origin of the Gaussians' frame (at any elevation)
    half = _camera_distance(o) * math.sin(0.5 * math.radians(o.opt.fovy)) if half is None else float(half)
    vol = gs_mesh.TsdfVolume(res, half, trunc=None if trunc is None else float(trunc), device=o.dev)
    fused = []
    for out, cv in itertools.chain([(o.out, o.cv)], (_orbit(o, float(e), True) for e in _setting(cfg, 'gs_mesh_elevations') or [])):
        depth, colour, cams = out["median_depth"][0, :, 0], _unpremultiplied(out, o.bg), cv[0]
        vol.integrate(depth, cams, o.renderer.tan_half_fov, colour=colour)
        if cfg.get('gs_mesh_texture'):
            fused.append((depth, colour, cams.to(depth.device)))
    rec['mesh_fused_views'] = vol.n_views
    verts, cols, faces = vol.extract()
    dropped, frac = "", _setting(cfg, 'gs_mesh_min_component')
    if frac is not None:
        verts, cols, faces, info = gs_mesh.drop_small_components(verts, cols, faces, min_fraction=float(frac))
        rec['mesh_components'], rec['mesh_components_dropped'] = info['components'], info['components'] - info['kept']
        dropped = (f"; {info['components']} components, {rec['mesh_components_dropped']} dropped with {info['dropped_faces']} faces "
                   f"and {info['dropped_vertices']} vertices")
    rec['mesh_ply'] = stem + '_gs_mesh.ply'
    rec['mesh_vertices'], rec['mesh_faces'] = gs_mesh.save_mesh_ply(verts, cols, faces, rec['mesh_ply'])
    rec['mesh_open_edges'] = gs_mesh.mesh_stats(verts, faces)['open_edges']
    logging.info(f"Save mesh ({rec['mesh_vertices']} vertices, {rec['mesh_faces']} faces, {rec['mesh_open_edges']} open edges; "
                 f"{res}^3 voxels of {vol.voxel:.5f}, {rec['mesh_fused_views']} views fused{dropped}) to {rec['mesh_ply']}")
    return verts, cols, faces, fused, vol.voxel


def _write_texture(cfg, o, stem, rec, verts, cols, faces, fused, voxel):
    """The same mesh as ``_gs_mesh.obj``: every fused view's colours baked over it, a texel seen within 2 voxels of a view's depth map"""
    if rec['mesh_faces'] == 0:
        logging.info("gs_mesh_texture: the mesh has no faces, no textured mesh is written")
        return
    patch = int(_setting(cfg, 'gs_mesh_texture_patch'))
    tex, uv, info = gs_mesh.bake_texture(verts, cols, faces, *(torch.cat([f[i] for f in fused]) for i in range(3)), o.renderer.tan_half_fov,
                                         patch=patch, depth_tol=2.0 * voxel)
    rec['mesh_obj'] = stem + '_gs_mesh.obj'
    gs_mesh.save_mesh_obj(verts, faces, uv, tex, stem + '_gs_mesh')
    rec['mesh_texture_size'], rec['mesh_texels_baked'] = info['size'], info['baked']
    logging.info(f"Save textured mesh ({info['size']} x {info['size']} texture, patch {patch}, {info['texels']} texels of faces, "
                 f"{100 * info['baked']:.1f} % baked from {len(fused) * o.n} views, {100 * info['fallback']:.1f} % vertex colours) "
                 f"to {rec['mesh_obj']}")


def _save_depth_maps(depth, npy_path, png_path, znear, zfar):
    """depth [n, S, S] (0 = no surface) -> the float32 .npy and an 8-bit sheet: znear .. zfar linearly white .. black, no surface black"""
    import numpy as np
    d = depth.numpy().astype(np.float32)
    np.save(npy_path, d)
    try:
        from PIL import Image
        shade = np.clip((zfar - d) / (zfar - znear), 0.0, 1.0)
        shade[d <= 0] = 0.0
        Image.fromarray(np.concatenate(list(np.round(shade * 255.0).astype(np.uint8)), axis=1)).save(png_path)
    except Exception as e:  # pragma: no cover
        logging.info(f'Step: save png error with {e}')


def _unpremultiplied(out, bg):
    """The colour of the surface in every view of ``out`` (GaussianRenderer.render_depth, sample 0), the background taken out:
    clamp((image - (1 - alpha) bg) / alpha, 0, 1) -> [V, 3, S, S]"""
    a = out["alpha"][0]
    return ((out["image"][0] - (1.0 - a) * bg) / a.clamp_min(1e-6)).clamp(0, 1)


def _export_points(cfg, o, stem, rec):
    """``_gs_points.ply``: the orbit's pixels that have a median depth, unprojected, coloured (``_unpremultiplied``), merged per voxel"""
    voxel, tan = _setting(cfg, 'gs_points_voxel'), o.renderer.tan_half_fov
    # default: 1/256 of the camera extent = the width the first orbit camera sees at its distance from the origin of the Gaussians' frame
    voxel = 2.0 * tan * _camera_distance(o) / 256.0 if voxel is None else float(voxel)
    colour, cam_view = _unpremultiplied(o.out, o.bg), o.cv[0]
    per_view = [gs.depth_to_points(o.out["median_depth"][0, v, 0], cam_view[v], tan) for v in range(cam_view.shape[0])]       # (points, pixels)
    pts = torch.cat([p for p, _ in per_view]).float().cpu()
    cols = torch.cat([colour[v].reshape(3, -1)[:, idx].t() for v, (_, idx) in enumerate(per_view)]).float().cpu()
    if pts.shape[0] > 0:
        pts, cols = gs.merge_points_voxel(pts, cols, voxel)
    rec['points_ply'] = stem + '_gs_points.ply'
    rec['points'] = gs.save_points_ply(pts, cols, rec['points_ply'])
    logging.info(f"Save point cloud ({rec['points']} points, voxel {voxel:.5f}) to {rec['points_ply']}")
