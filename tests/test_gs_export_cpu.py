"""3-D export without a GPU: the .ply writer / reader (GaussianRenderer.save_ply / load_ply, the layout of the reference's
core/gs.py:97-186) against an independent reader, orbit cameras in the generation set's frame, and the entrance keys
(save_gaussians & co.) on the CPU plan interpreter."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from tests import plan_interp

NAMES = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]


def _gaussians(n, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g) - 0.5
    op = torch.rand(n, 1, generator=g)
    op[::7] = 0.001                                                # below the 0.005 pruning threshold
    op[1] = 0.005                                                  # at it: kept (>=)
    sc = 0.01 + 0.1 * torch.rand(n, 3, generator=g)
    rot = torch.randn(n, 4, generator=g)
    rgb = torch.rand(n, 3, generator=g)
    return torch.cat([pos, op, sc, rot, rgb], dim=1).unsqueeze(0)


def _read_ply(path):
    """Independent reader: header lines, then little-endian float32 rows."""
    with open(path, "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")[:-1] + ["end_header"]
    n = int(lines[2].split()[2])
    rows = [struct.unpack("<14f", body[56 * i:56 * (i + 1)]) for i in range(n)]
    return lines, np.array(rows, dtype=np.float32).reshape(n, 14), len(body)


def test_ply_header_body_activations_and_pruning(tmp_path):
    from videomv_amd.gs import GaussianRenderer
    g = _gaussians(50, 1)
    path = str(tmp_path / "a.ply")
    n = GaussianRenderer(64).save_ply(g, path)
    lines, rows, nbytes = _read_ply(path)
    keep = g[0, :, 3] >= 0.005
    assert n == int(keep.sum()) == rows.shape[0] and 0 < n < 50 and nbytes == 56 * n
    assert lines == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property float {p}" for p in NAMES] + ["end_header"]
    k = g[0][keep].double()
    o = k[:, 3].clamp(1e-6, 1 - 1e-6)
    want = torch.cat([k[:, 0:3], (k[:, 11:14] - 0.5) / 0.28209479177387814, torch.log(o / (1 - o)).unsqueeze(1), torch.log(k[:, 4:7] + 1e-8),
                      k[:, 7:11]], dim=1)
    assert np.allclose(rows, want.numpy(), rtol=1e-5, atol=1e-5)
    # compatible=False: the activated values as they are
    GaussianRenderer(64).save_ply(g, path, compatible=False)
    _, raw, _ = _read_ply(path)
    assert np.array_equal(raw[:, 6], g[0][keep][:, 3].numpy()) and np.array_equal(raw[:, 7:10], g[0][keep][:, 4:7].numpy())


@pytest.mark.parametrize("compatible", [True, False])
def test_ply_round_trip(tmp_path, compatible):
    from videomv_amd.gs import GaussianRenderer
    g = _gaussians(200, 2)
    path = str(tmp_path / "b.ply")
    GaussianRenderer(64).save_ply(g, path, compatible=compatible)
    back = GaussianRenderer.load_ply(path, compatible=compatible)
    kept = g[0][g[0, :, 3] >= 0.005]
    assert back.shape == kept.shape and back.dtype == torch.float32
    assert float((back - kept).abs().max()) <= 1e-5


def _centres(cam_view):
    """camera centres of row-vector cam_view matrices [V, 4, 4]"""
    return torch.inverse(cam_view.double().transpose(-1, -2))[:, :3, 3]


def test_orbit_cameras_live_in_the_generation_frame():
    from videomv_amd.camera import entrance_camera_data
    from videomv_amd.lgm import prepare_gs_data, orbit_cameras, LgmOptions
    opt = LgmOptions()
    gen = entrance_camera_data(24, elevation=15, camera_distance=2.0)
    gs = prepare_gs_data(gen, opt)
    cv, cvp = orbit_cameras(gen, 24, 15, 2.0, opt)
    assert cv.shape == cvp.shape == (1, 24, 4, 4)
    assert torch.allclose(cv, gs["cam_view"], atol=1e-6) and torch.allclose(cvp, gs["cam_view_proj"], atol=1e-6)
    # another elevation: same frame — every camera sits at the orbit distance from the generation orbit's centre (the world origin
    # in the generation frame, where every generation camera is 2.0 away too), and the first camera is 15 degrees above the
    # generation set's first one about that centre, not moved onto it
    gen_c = _centres(gs["cam_view"][0])
    cv30, cvp30 = orbit_cameras(gen, 8, 30, 2.0, opt)
    c = _centres(cv30[0])
    o = c - c.mean(0)
    axis = torch.linalg.cross(o[0], o[2])
    axis = axis / axis.norm()
    gaxis = torch.linalg.cross(gen_c[0] - gen_c.mean(0), gen_c[6] - gen_c.mean(0))
    assert abs(abs(float(torch.dot(axis, gaxis / gaxis.norm()))) - 1.0) < 1e-6           # the same orbit axis
    # the common sphere centre: on that axis, 2.0 from every camera of both sets
    t = (4.0 - ((gen_c[0] - gen_c.mean(0)) ** 2).sum()).sqrt()
    cands = [gen_c.mean(0) + s_ * t * axis for s_ in (1.0, -1.0)]
    centre = min(cands, key=lambda p: float(((c - p).norm(dim=1) - 2.0).abs().max()))
    assert torch.allclose((c - centre).norm(dim=1), torch.full((8,), 2.0, dtype=torch.float64), atol=1e-5)
    assert torch.allclose((gen_c - centre).norm(dim=1), torch.full((24,), 2.0, dtype=torch.float64), atol=1e-5)
    c0 = gen_c[0]
    u, w = c[0] - centre, c0 - centre
    ang = math.degrees(math.acos(float(torch.dot(u, w) / (u.norm() * w.norm()))))
    assert abs(ang - 15.0) < 1e-3
    own = prepare_gs_data(entrance_camera_data(8, elevation=30, camera_distance=2.0), opt)       # normalised to ITS first camera
    assert torch.allclose(_centres(own["cam_view"][0])[0], c0, atol=1e-5) and not torch.allclose(cv30, own["cam_view"], atol=1e-3)


def _tiny_cfg(tmp_path, extra):
    from videomv_amd.config import Config
    tmp_path.mkdir(parents=True, exist_ok=True)
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("a wooden chair\n")
    argv = ["--cfg", "configs/t2v_infer.yaml", "--debug", "device", "cpu", "allow_random_init", "True", "num_views", "4",
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


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("extra", [["UNet.use_lgm_refine", "False"], ["resolution", "[64, 32]"]])
def test_save_gaussians_fails_before_sampling(monkeypatch, tmp_path, extra):
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    import videomv_amd.entrance  # noqa: F401
    cu = _tiny_cfg(tmp_path, ["save_gaussians", "True"] + extra)
    if extra[0] == "resolution":
        cu.cfg_dict["resolution"] = [64, 32]
    with pytest.raises(Exception, match="save_gaussians"):      # (the registry re-raises as Exception)
        INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    assert not os.path.exists(tmp_path / "out")                     # nothing sampled, nothing written


def test_entrance_writes_a_loadable_ply_and_nothing_else_changes(monkeypatch, tmp_path):
    """The LGM-refined loop with 2 DDIM steps (no refined step runs; the LGM weights exist) and save_gaussians: <stem>_gs.ply loads;
    the run without the keys writes exactly the files of the run with them minus the .ply, and the same latents."""
    plan_interp.install(monkeypatch)
    from videomv_amd.registry import INFER_ENGINE
    from videomv_amd.gs import GaussianRenderer
    import videomv_amd.entrance  # noqa: F401
    cfgs = {}
    for name, extra in (("plain", []), ("export", ["save_gaussians", "True", "gs_fit_iters", "0"])):
        cu = _tiny_cfg(tmp_path / name, extra)
        cfgs[name] = INFER_ENGINE.build(dict(type=cu.TASK_TYPE), cfg_update=cu.cfg_dict)
    plain, export = (_files(cfgs[k].log_dir) for k in ("plain", "export"))
    plys = [f for f in export if f.endswith("_gs.ply")]
    assert len(plys) == 1 and [f for f in export if f not in plys] == plain
    assert "gs_exports" not in cfgs["plain"]
    rec, = cfgs["export"].gs_exports
    g = GaussianRenderer.load_ply(rec["ply"])
    assert g.shape == (rec["vertices"], 14) and 0 < g.shape[0] <= 4 * 64 * 64 and torch.isfinite(g).all()
    for f in plain:
        if f.endswith(".pt"):
            a, b = (torch.load(os.path.join(cfgs[k].log_dir, f)) for k in ("plain", "export"))
            assert torch.equal(a["latent"], b["latent"])


def test_the_settings_table_and_the_documented_defaults_agree():
    """config.default_cfg documents every export key with its default; the table the check and the stages read holds the same value"""
    from videomv_amd.config import default_cfg
    from videomv_amd.gs_export import SETTINGS
    cfg = default_cfg()
    assert {k: cfg[k] for k in SETTINGS} == {k: s.default for k, s in SETTINGS.items()}
