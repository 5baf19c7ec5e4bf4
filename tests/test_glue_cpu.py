"""The float64 glue references (tests/glue_ref.py) pinned without a GPU: against the independent statements of the same operations in
oracle/ and torch.nn.functional, and against the fp32 interpreter (tests/plan_interp.py) at the bound the GPU test holds the kernels to —
two hands, one header.  The last test shows the bound has teeth: a reference coefficient off by 1e-5 is caught."""
import pytest
import torch
import torch.nn.functional as Fn

from videomv_amd import _lib as L
from tests import glue_ref as G
from tests import plan_interp as I

BF = L.elem()
D = torch.float64


def close(a, b, tol=1e-12):
    scale = float(b.abs().max().clamp_min(1e-30))
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


# ------------------------------------------------------------------------------------------------- against the oracle's statements
def test_glue_ref_posterior_matches_vae_ref():
    from oracle.vae_ref import posterior_sample
    n, zc, HW, ld = 2, 4, 37, 12
    t = G.posterior_inputs(n, zc, HW, ld)
    R = G.posterior_sample(t["moments_rows"], ld, t["noise"], n, zc, HW, 0.18215)
    mom = t["moments_rows"].double().view(n, HW, ld)[:, :, :2 * zc].permute(0, 2, 1).reshape(n, 2 * zc, 1, HW)
    want = posterior_sample(mom, t["noise"].double().view(n, zc, 1, HW), G.f32(0.18215))
    close(R.ref, want.reshape(n, zc, HW))
    assert bool((R.mag >= R.ref.abs() * (1 - 1e-12)).all())


def _oracle_step(betas, y, u, xt, mean_type, clamp, eta, noise):
    """one step of the oracle's loop (ddim_timesteps = 1: t = 1, a_prev = abar_0) in float64 on tables rounded to fp32 -> (x_{t-1}, coefficients)"""
    from oracle.ddim_ref import DDIMTables, ddim_sample_loop
    tb = DDIMTables(betas)
    for k in ("ac", "sqrt_ac", "sqrt_1mac", "sqrt_recip", "sqrt_recipm1"):
        setattr(tb, k, getattr(tb, k).float().double())
    model = lambda x, t, out: out
    nx = ddim_sample_loop(xt[None], model, tb, [dict(out=y[None]), dict(out=u[None])], G.f32(9.0), ddim_timesteps=1, mean_type=mean_type, eta=eta,
                          clamp=clamp, step_noise=lambda i, x: noise[None])[0]
    a_t, a_prev = tb.ac[1], tb.ac[0]
    sigma = float(eta * torch.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)))
    return nx, dict(c_recip=float(tb.sqrt_recip[1]), c_recipm1=float(tb.sqrt_recipm1[1]), c_sqrt_ac=float(tb.sqrt_ac[1]), c_sqrt_1mac=float(tb.sqrt_1mac[1]),
                    a_prev=float(a_prev), sigma=sigma)


@pytest.mark.parametrize("mean_type,clamp,eta", [("eps", None, 0.0), ("v", None, 0.0), ("eps", 1.0, 0.0), ("v", 0.7, 0.6), ("eps", None, 1.0)])
@pytest.mark.parametrize("tables", ["last-of-1000", "coarse"])
def test_glue_ref_ddim_matches_one_oracle_step(tables, mean_type, clamp, eta):
    """cfg_ddim_step (eps / v prediction, clamp, eta > 0) and ddim_x0_step against oracle/ddim_ref.ddim_sample_loop through a model that returns
    fixed predictions.  The only difference is sigma's rounding to the `float` of the C ABI: 1e-6 of the magnitude."""
    from oracle.ddim_ref import betas_for
    betas = betas_for("linear_sd") if tables == "last-of-1000" else betas_for("linear_sd", num_timesteps=10, init_beta=0.2, last_beta=0.5)
    Cc, F_, HW, ld = 4, 3, 37, 8
    t = G.cfg_ddim_inputs(Cc, F_, HW, ld)
    e = t["eps_rows"].double().view(2, F_ * HW, ld)[:, :, :Cc]
    y, u = e[0].t().reshape(Cc, F_, HW), e[1].t().reshape(Cc, F_, HW)
    xt, noise = t["xt"].double(), t["noise"].double()
    want, c = _oracle_step(betas, y, u, xt, mean_type, clamp, eta, noise)
    R, R0 = G.cfg_ddim_step(t["eps_rows"], ld, t["xt"], 9.0, v_pred=mean_type == "v", clamp=clamp or 0.0, noise=t["noise"] if eta else None, **c)
    assert float(((R.ref - want).abs() / R.mag).max()) < 1e-6
    if clamp:
        assert float(R0.ref.abs().max()) == G.f32(clamp)
    if mean_type == "eps":          # CFG on the two branches' x0 is CFG on their eps: the LGM-refined step's form of the same update
        cr, crm1 = c["c_recip"], c["c_recipm1"]
        Rx = G.ddim_x0_step(cr * xt - crm1 * y, cr * xt - crm1 * u, xt, 9.0, cr, crm1, c["a_prev"], clamp=clamp or 0.0, sigma=c["sigma"], noise=noise if eta else None)
        assert float(((Rx.ref - want).abs() / Rx.mag).max()) < 1e-6


@pytest.mark.parametrize("n,zero_rot", [(255, False), (300, True)])
def test_glue_ref_gaussian_activation_matches_lgm_ref(n, zero_rot):
    from oracle.lgm_ref import gaussian_activation
    raw = G.gaussian_inputs(n, zero_rot)
    R = G.gaussian_activation(raw, n)
    close(R.ref, gaussian_activation(raw[None, :, :14].double())[0])
    assert G.gaussian_rot_sum_depth(70001) == 2 + 8 + 256 and G.gaussian_rot_sum_depth(255) == 1 + 8 + 1


@pytest.mark.parametrize("F_,big", [(1, False), (24, False), (64, True)])
def test_glue_ref_adapter_matches_unet_i2v_ref(F_, big):
    from oracle.unet_i2v_ref import temporal_adapter
    HW = 11
    x = G.rnd((F_ * HW, 4), 1).to(BF)
    w = G.adapter_weights(big)
    R = G.i2v_temporal_adapter(x, w, F_, HW, 2.0)
    assert F_ == 1 or (G.i2v_temporal_adapter.score_max > 40.0) == big
    wd, p = w.double(), "local_temporal_encoder.layers.0"
    sd = {f"{p}.0.norm.weight": wd[0:4], f"{p}.0.norm.bias": wd[4:8], f"{p}.0.fn.to_qkv.weight": wd[8:104].view(24, 4),
          f"{p}.0.fn.to_out.0.weight": wd[104:136].view(4, 8), f"{p}.0.fn.to_out.0.bias": wd[136:140], f"{p}.1.net.0.0.weight": wd[140:204].view(16, 4),
          f"{p}.1.net.0.0.bias": wd[204:220], f"{p}.1.net.2.weight": wd[220:284].view(4, 16), f"{p}.1.net.2.bias": wd[284:288]}
    want = 2.0 * temporal_adapter(sd, x.double().view(F_, HW, 4).permute(1, 0, 2))
    close(R.ref, want.permute(1, 0, 2).reshape(F_ * HW, 4), 1e-11)
    assert bool((R.extra > 0).all())


@pytest.mark.parametrize("IH,IW,OH,OW", [(9, 14, 4, 4), (5, 5, 8, 8), (6, 7, 6, 7), (40, 54, 48, 44)])
def test_glue_ref_avgpool_matches_torch(IH, IW, OH, OW):
    n, Cc = 2, 8
    x = G.rnd((n * IH * IW, Cc), 3).to(BF)
    R = G.adaptive_avgpool_rows(x, n, Cc, IH, IW, OH, OW)
    want = Fn.adaptive_avg_pool2d(x.double().view(n, IH, IW, Cc).permute(0, 3, 1, 2), (OH, OW)).permute(0, 2, 3, 1).reshape(n * OH * OW, Cc)
    close(R.ref, want)


@pytest.mark.parametrize("S_in,S", [(80, 32), (384, 296), (64, 64), (48, 96)])
def test_glue_ref_render_to_vae_matches_interpolate(S_in, S):
    img = torch.rand(2, 3, S_in, S_in, generator=G.g(2))
    want = (Fn.interpolate(img.double(), size=(S, S), mode="nearest") - 0.5) / 0.5
    assert torch.equal(G.lgm_render_to_vae(img, S), want)


def test_glue_ref_layouts_and_embeddings_match_plain_indexing():
    """the layout references against element-by-element statements of the header's index formulas; sinusoidal against the oracle's"""
    from oracle.unet_ref import sinusoidal_embedding
    nb, Cc, F_, H, W, nrep, Cpad = 2, 3, 2, 2, 3, 2, 5
    x = G.rnd((nb, Cc, F_, H, W), 4)
    rows = G.latent_to_rows(x, Cpad, nrep)
    per = nb * F_ * H * W
    for rep in range(nrep):
        for b in range(nb):
            for f in range(F_):
                for p in range(H * W):
                    r = rows[rep * per + (b * F_ + f) * H * W + p]
                    assert r[:Cc].tolist() == x[b, :, f].reshape(Cc, -1)[:, p].double().tolist() and r[Cc:].abs().sum() == 0
    r2 = G.rnd((2 * 6, 5), 3)
    out = G.rows_to_nchw(r2, 2, 3, 6)
    assert all(float(out[i, c, p]) == float(r2[i * 6 + p, c]) for i in range(2) for c in range(3) for p in range(6))
    t = torch.tensor([0.0, 1.0, 981.0, 999.0])
    for dim in (320, 37):
        G.check(f"oracle.sinusoidal[{dim}]", sinusoidal_embedding(t, dim), G.sinusoidal(t, dim), G.K["sinusoidal"])          # (the oracle computes in fp32)


# ------------------------------------------------------------------------------------------------- against the fp32 interpreter
def _interp_cfg(variant, HW, c_over=None):
    coef, v_pred, clamp = G.DDIM_VARIANTS[variant]
    Cc, F_, ld = 4, 3, 8
    c = G.ddim_coef(coef)
    t = G.cfg_ddim_inputs(Cc, F_, HW, ld)
    noise = t["noise"] if c["sigma"] > 0 else None
    R = G.cfg_ddim_step(t["eps_rows"], ld, t["xt"], 9.0, v_pred=v_pred, clamp=clamp, noise=noise, **dict(c, **(c_over or {})))
    xt, x0 = t["xt"].clone().view(1, Cc, F_, 1, HW), torch.zeros(1, Cc, F_, 1, HW)
    I.cfg_ddim_step(t["eps_rows"], ld, xt, 9.0, v_pred=v_pred, x0_out=x0, clamp=clamp, noise=noise.view(1, Cc, F_, 1, HW) if noise is not None else None, **c)
    return xt, x0, R


@pytest.mark.parametrize("variant", list(G.DDIM_VARIANTS))
def test_glue_interp_cfg_ddim_step(variant):
    xt, x0, (R_xt, R_x0) = _interp_cfg(variant, 37)
    G.check(f"interp.cfg_ddim_step[{variant}].xt", xt, R_xt, G.K["cfg_ddim_step"])
    G.check(f"interp.cfg_ddim_step[{variant}].x0_out", x0, R_x0, G.K["cfg_ddim_step.x0_out"])


def _interp_x0(variant, n, cr_scale=1.0):
    coef, _, clamp = G.DDIM_VARIANTS[variant]
    c = G.ddim_coef(coef)
    t = G.ddim_x0_inputs(n)
    noise = t["noise"] if c["sigma"] > 0 else None
    R = G.ddim_x0_step(t["x0_cond"], t["x0_uncond"], t["xt"], 9.0, c["c_recip"] * cr_scale, c["c_recipm1"], c["a_prev"], clamp=clamp, sigma=c["sigma"], noise=noise)
    xt = t["xt"].clone()
    I.ddim_x0_step(t["x0_cond"], t["x0_uncond"], xt, 9.0, c["c_recip"], c["c_recipm1"], c["a_prev"], clamp=clamp or None, sigma=c["sigma"], noise=noise)
    return xt, R


@pytest.mark.parametrize("variant", [v for v, s in G.DDIM_VARIANTS.items() if not s[1]])
def test_glue_interp_ddim_x0_step(variant):
    xt, R = _interp_x0(variant, 445)
    G.check(f"interp.ddim_x0_step[{variant}]", xt, R, G.K["ddim_x0_step"])


def _interp_views(branch, crm1_scale=1.0):
    Cc, F_, HW, ld, idx4 = 4, 5, 37, 8, (4, 0, 2, 2)
    c = G.ddim_coef("last" if branch else "mid")
    eps, xt = G.nan_pad(G.rnd((2 * F_ * HW, Cc), 1), ld), G.rnd((Cc, F_, HW), 2)
    R = G.lgm_x0_views(eps, ld, branch, xt, idx4, c["c_recip"], c["c_recipm1"] * crm1_scale, 1.0 / 0.18215)
    out = torch.zeros(4, Cc, 1, HW)
    I.lgm_x0_views(eps, ld, branch, xt.view(1, Cc, F_, 1, HW), idx4, c["c_recip"], c["c_recipm1"], G.f32(1.0 / 0.18215), out)
    return out, R


def _interp_pack():
    V, HW = 3, 37
    dec, rays = G.rnd((V, 3, HW), 1, 1.2), G.rnd((V, 6, HW), 2)
    out = torch.zeros(V, 9, 1, HW)
    I.lgm_pack_input(dec.view(V, 3, 1, HW), rays.view(V, 6, 1, HW), out)
    return out, dec, rays


def _interp_posterior(scale_ref=0.18215):
    n, zc, HW, ld = 2, 4, 37, 12
    t = G.posterior_inputs(n, zc, HW, ld)
    R = G.posterior_sample(t["moments_rows"], ld, t["noise"], n, zc, HW, scale_ref)
    z = torch.zeros(n, zc, 1, HW)
    I.posterior_sample(t["moments_rows"], ld, t["noise"].view(n, zc, 1, HW), z, G.f32(0.18215))
    return z, R


def _interp_sinusoidal(dim, base=10000.0):
    t = torch.tensor([0.0, 1.0, 981.0, 999.0])
    out = torch.zeros(4, dim, dtype=BF)
    I.sinusoidal(t, out, 4, dim)
    return out, G.sinusoidal(t, dim, base)


def test_glue_interp_lgm_posterior_embeddings():
    for branch in (0, 1):
        out, R = _interp_views(branch)
        G.check(f"interp.lgm_x0_views[b{branch}]", out, R, G.K["lgm_x0_views"])
    out, dec, rays = _interp_pack()
    G.check("interp.lgm_pack_input", out, G.lgm_pack_input(dec, rays), G.K["lgm_pack_input"])
    z, R = _interp_posterior()
    G.check("interp.posterior_sample", z, R, G.K["posterior_sample"])
    for rows, Cc, rpt, cam_rows in ((37, 40, 5, 5), (37, 40, 5, 0)):
        temb, cam = G.rnd((-(-rows // rpt), Cc), 1, 2.0), (G.rnd((cam_rows, Cc), 2, 2.0) if cam_rows else None)
        out = torch.zeros(rows, Cc, dtype=BF)
        I.emb_combine_silu(temb, cam, out, rows, Cc, rpt, cam_rows)
        G.check(f"interp.emb_combine_silu[cam={cam_rows}]", out, G.emb_combine_silu(temb, cam, rows, Cc, rpt, cam_rows), G.K["emb_combine_silu"], BF)
    for dim in (320, 37):
        out, R = _interp_sinusoidal(dim)
        G.check(f"interp.sinusoidal[{dim}]", out, R, G.K["sinusoidal"], BF)
        assert dim % 2 == 0 or bool((out[:, -1] == 0).all())


def test_glue_interp_layout():
    nb, Cc, F_, H, W, nrep = 2, 4, 3, 1, 37, 2
    x = G.rnd((nb, Cc, F_, H, W), 4)
    rows = torch.full((nrep * nb * F_ * H * W, 8), 7.0, dtype=BF)
    I.latent_to_rows(x, rows, 8, nrep)
    assert torch.equal(rows, G.latent_to_rows(x, 8, nrep).float().to(BF))
    I.latent_to_rows_keep(x, rows.fill_(7.0), 8, nrep)
    assert torch.equal(rows[:, :Cc], G.latent_to_rows_keep(x, nrep).float().to(BF)) and bool((rows[:, Cc:] == 7).all())
    for ld, dt in ((4, torch.float32), (8, BF)):
        r = G.nan_pad(G.rnd((3 * 37, 3), 3), ld).to(dt)
        out = torch.zeros(3, 3, 1, 37)
        I.rows_to_nchw(r, ld, out)
        assert torch.equal(out.view(3, 3, 37), G.rows_to_nchw(r, 3, 3, 37).float())
    img = torch.rand(3, 3, 80, 80, generator=G.g(2))
    out = torch.zeros(3, 3, 32, 32)
    I.lgm_render_to_vae(img, out)
    assert torch.equal(out, G.lgm_render_to_vae(img, 32).float())


@pytest.mark.parametrize("F_,big", [(1, False), (24, False), (64, False), (24, True), (64, True)])
def test_glue_interp_i2v_temporal_adapter(F_, big):
    HW, nrep = 11, 2
    x, w = G.rnd((F_ * HW, 4), 1).to(BF), G.adapter_weights(big)
    out = torch.zeros(nrep * F_ * HW, 8, dtype=BF)
    I.i2v_temporal_adapter(x, 4, out.data_ptr() + 8, 8, w, F_, HW, nrep, 2.0)
    R = G.i2v_temporal_adapter(x, w, F_, HW, 2.0)
    for rep in range(nrep):
        G.check(f"interp.i2v_temporal_adapter[F{F_}{'-big' if big else ''}]", out[rep * F_ * HW:(rep + 1) * F_ * HW, 4:], R, 0, BF)
    assert bool((out[:, :4] == 0).all())


@pytest.mark.parametrize("IH,IW,OH,OW", [(9, 14, 4, 4), (5, 5, 8, 8), (6, 7, 6, 7)])
def test_glue_interp_adaptive_avgpool_rows(IH, IW, OH, OW):
    n, Cc = 2, 32
    x = G.rnd((n * IH * IW, Cc), 3).to(BF)
    y = torch.zeros(n * OH * OW, Cc, dtype=BF)
    I.adaptive_avgpool_rows(x, Cc, y, Cc, n, Cc, IH, IW, OH, OW)
    G.check(f"interp.adaptive_avgpool_rows[{IH}x{IW}->{OH}x{OW}]", y, G.adaptive_avgpool_rows(x, n, Cc, IH, IW, OH, OW), 0, BF)


@pytest.mark.parametrize("n,zero_rot", [(1, False), (255, False), (65537, False), (255, True)])
def test_glue_interp_gaussian_activation(n, zero_rot):
    raw = G.gaussian_inputs(n, zero_rot)
    out = torch.zeros(n, 14)
    I.gaussian_activation(torch.nan_to_num(raw), 16, out, n, None)
    G.check(f"interp.gaussian_activation[{n}]", out, G.gaussian_activation(raw, n), 0)


# ------------------------------------------------------------------------------------------------- the bound has teeth
def test_glue_bound_catches_a_coefficient_off_by_1e_5(monkeypatch):
    """each reference with ONE coefficient off by 1e-5 relative no longer agrees with the interpreter at the derived bound — at the mid-schedule
    coefficients and at the last step's, where the bound carries no conditioning term at all.  The inputs are built outside the `raises`
    blocks and the message is matched, so only the bound itself can satisfy them."""
    p = 1.0 + 1e-5
    beyond = dict(match="beyond the bound")
    for variant in ("eps", "eps-last"):
        c = G.ddim_coef(G.DDIM_VARIANTS[variant][0])
        xt, _, (R, _) = _interp_cfg(variant, 37, dict(c_recip=c["c_recip"] * p))
        with pytest.raises(AssertionError, **beyond):
            G.check(f"perturbed.cfg_ddim_step[{variant}]", xt, R, G.K["cfg_ddim_step"])
        xt, R = _interp_x0(variant, 445, p)
        with pytest.raises(AssertionError, **beyond):
            G.check(f"perturbed.ddim_x0_step[{variant}]", xt, R, G.K["ddim_x0_step"])
    c = G.ddim_coef("mid")
    _, x0, (_, R0) = _interp_cfg("v", 37, dict(c_sqrt_1mac=c["c_sqrt_1mac"] * p))          # (x0's weight in x_{t-1}, sa - sb / crm1, nearly cancels: x0_out shows it)
    with pytest.raises(AssertionError, **beyond):
        G.check("perturbed.cfg_ddim_step[v].x0_out", x0, R0, G.K["cfg_ddim_step.x0_out"])
    out, R = _interp_views(0, p)
    with pytest.raises(AssertionError, **beyond):
        G.check("perturbed.lgm_x0_views", out, R, G.K["lgm_x0_views"])
    z, R = _interp_posterior(0.18215 * p)
    with pytest.raises(AssertionError, **beyond):
        G.check("perturbed.posterior_sample", z, R, G.K["posterior_sample"])
    out, R = _interp_sinusoidal(320, 10000.0 * p)
    with pytest.raises(AssertionError, **beyond):
        G.check("perturbed.sinusoidal", out, R, G.K["sinusoidal"], BF)
    out, dec, rays = _interp_pack()
    monkeypatch.setattr(G, "IMAGENET_STD", (0.229 * p, 0.224, 0.225))
    R = G.lgm_pack_input(dec, rays)
    with pytest.raises(AssertionError, **beyond):
        G.check("perturbed.lgm_pack_input", out, R, G.K["lgm_pack_input"])
