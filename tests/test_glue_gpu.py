"""Every sampler / LGM glue kernel of csrc/elementwise.hip against its float64 reference (tests/glue_ref.py) — `pytest -m gpu`.

Shapes: for every kernel an under-cap twin with odd sizes (HW = 37) and one whose element count is 8192 * 256 + a ragged remainder, so that
the grid-stride loop runs a second, partial pass and every `long` index expression is evaluated beyond the first.  Sources with a row
stride are NaN outside the columns the contract reads.

Comparison.  Layout kernels and vmv_lgm_render_to_vae: bit for bit (the fp32 value, or its rounding to the library's element type).
Arithmetic kernels: every element, no exclusion,

    |got - ref| <= 2^-24 * (k * mag + extra)  [+ half an ulp of the element type at ref, for 16-bit outputs]

with mag / extra from glue_ref and k the number of fp32 roundings that flow into an element (each is at most 2^-24 of a term of mag),
derived in each test's docstring from the operation named by include/vmv.h — not from a run of the kernels.  Units: one rounding = 1; a
fast exponential = 1 + |arg| log2 e (in `extra`); a call of sinf / cosf / powf / tanhf / log1pf / expf = 4 units (the issue's count: 2 ulp); a
correctly rounded division or square root = 1; a hardware reciprocal or reciprocal square root (1 ulp) = 2.  Each case prints the measured
maximum of |got - ref| / (2^-24 mag).
"""
import pytest
import torch

from videomv_amd import _lib as L
from videomv_amd import ops
from tests import glue_ref as G

pytestmark = pytest.mark.gpu
BF = L.elem()
D = torch.float64
PAST = G.CAP          # 2 097 152


def report(name, got, R, k, out16=False):
    """assert the bound on every element; print the measured ratio"""
    G.check(name, got, R, k, BF if out16 else None, L.elem_name())


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def to_elem(ref64):
    """the 16-bit rounding of an fp32 value, made with the library's own element type"""
    return ref64.to(torch.float32).to(BF)


# ------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("nb,Cc,F_,H,W,nrep", [(2, 4, 3, 1, 37, 2), (2, 4, 3, 7, 49933, 2)], ids=["under", "past-cap"])
def test_glue_latent_to_rows(nb, Cc, F_, H, W, nrep):
    """vmv_latent_to_rows and vmv_latent_to_rows_keep, nb_src = 2: bit-exact; _keep leaves columns [C, ld) as they were"""
    x = G.rnd((nb, Cc, F_, H, W), 4)
    per = nb * F_ * H * W
    assert (per > PAST) == (W > 37)
    rows = torch.full((nrep * per, 8), 7.0, dtype=BF, device="cuda")
    ops.latent_to_rows(x.cuda(), rows, 8, nrep)
    assert torch.equal(bits16(rows), bits16(to_elem(G.latent_to_rows(x, 8, nrep))))
    keep = torch.full((nrep * per, 8), 7.0, dtype=BF, device="cuda")
    ops.latent_to_rows_keep(x.cuda(), keep, 8, nrep)
    want = torch.full((nrep * per, 8), 7.0, dtype=BF)
    want[:, :Cc] = to_elem(G.latent_to_rows_keep(x, nrep))
    assert torch.equal(bits16(keep), bits16(want))


@pytest.mark.parametrize("n,Cc,HW", [(3, 3, 37), (3, 3, 233113)], ids=["under", "past-cap"])
@pytest.mark.parametrize("kind", ["f32-ld4", "elem-ld8"])
def test_glue_rows_to_nchw(kind, n, Cc, HW):
    """vmv_rows_to_nchw from fp32 rows (ld 4) and element-type rows (ld 8), NaN in the columns past C: bit-exact"""
    ld = 4 if kind == "f32-ld4" else 8
    rows = G.nan_pad(G.rnd((n * HW, Cc), 3), ld)
    if kind != "f32-ld4":
        rows = rows.to(BF)
    out = torch.full((n, Cc, 1, HW), 7.0, device="cuda")
    ops.rows_to_nchw(rows.cuda(), ld, out)
    assert torch.equal(out.cpu().reshape(n, Cc, HW), G.rows_to_nchw(rows, n, Cc, HW).float())


@pytest.mark.parametrize("V,S_in,S", [(3, 80, 32), (8, 384, 296)], ids=["under", "past-cap"])
def test_glue_lgm_render_to_vae(V, S_in, S):
    """vmv_lgm_render_to_vae at non-integer size ratios: the fp32 rounding of (x - 0.5) / 0.5 at the floor(dst * S_in / S) source, bit-exact"""
    assert (V * 3 * S * S > PAST) == (S == 296)
    img = torch.rand(V, 3, S_in, S_in, generator=G.g(2))
    out = torch.full((V, 3, S, S), 7.0, device="cuda")
    ops.lgm_render_to_vae(img.cuda(), out)
    assert torch.equal(out.cpu(), G.lgm_render_to_vae(img, S).float())


# ------------------------------------------------------------------------------------------------- DDIM
def _clamp_shares(x0, clamp):
    clamp = G.f32(clamp)
    lo, hi = float((x0 <= -clamp).double().mean()), float((x0 >= clamp).double().mean())
    assert lo > 0.05 and hi > 0.05 and lo + hi < 0.95, (lo, hi)          # the clamp is active in both directions and idle elsewhere


# every variant under the cap; one stochastic clamped case and the cancelling last step past it
@pytest.mark.parametrize("variant,HW", [(v, 37) for v in G.DDIM_VARIANTS] + [("v-clamp-eta", 174791), ("eps-last", 174791)])
def test_glue_cfg_ddim_step(variant, HW):
    """vmv_cfg_ddim_step, C = 4, F = 3, eps rows of stride 8 with NaN pad.  k (xt) = 16, every rounding that flows into an element: the CFG
    mix u + g (y - u) 3, x0 = a xt - b out 3, cr xt 1, the subtraction 1, the division 1, sqrt(q) 1 (q's own cancellation is in `extra`),
    sb eps 1, sqrt(a_prev) 1, sa x0 1, sigma noise 1, the two additions 2.  k (x0_out) = 6: the mix 3 and x0 3; the clamp is exact."""
    coef, v_pred, clamp = G.DDIM_VARIANTS[variant]
    Cc, F_, ld = 4, 3, 8
    assert (Cc * F_ * HW > PAST) == (HW > 37)
    c = G.ddim_coef(coef)
    t = G.cfg_ddim_inputs(Cc, F_, HW, ld)
    noise = t["noise"] if c["sigma"] > 0 else None
    R_xt, R_x0 = G.cfg_ddim_step(t["eps_rows"], ld, t["xt"], 9.0, v_pred=v_pred, clamp=clamp, noise=noise, **c)
    if clamp:
        _clamp_shares(R_x0.ref, clamp)
    xt = t["xt"].reshape(1, Cc, F_, 1, HW).cuda()
    x0 = torch.full_like(xt, 7.0)
    ops.cfg_ddim_step(t["eps_rows"].cuda(), ld, xt, 9.0, v_pred=v_pred, x0_out=x0, clamp=clamp, noise=noise.cuda() if noise is not None else None, **c)
    report(f"cfg_ddim_step[{variant}-{HW}].xt", xt, R_xt, G.K["cfg_ddim_step"])
    report(f"cfg_ddim_step[{variant}-{HW}].x0_out", x0, R_x0, G.K["cfg_ddim_step.x0_out"])
    if variant == "eps":          # x0_out is optional
        xt2 = t["xt"].reshape(1, Cc, F_, 1, HW).cuda()
        ops.cfg_ddim_step(t["eps_rows"].cuda(), ld, xt2, 9.0, v_pred=v_pred, **c)
        assert torch.equal(xt2, xt)


@pytest.mark.parametrize("variant,n", [(v, 445) for v, s in G.DDIM_VARIANTS.items() if not s[1]] + [("eps-eta", PAST + 300), ("eps-last-clamp", PAST + 300)])
def test_glue_ddim_x0_step(variant, n):
    """vmv_ddim_x0_step, in place.  k = 13, every rounding that flows into an element: the CFG mix of the two x0 3, cr xt 1, the subtraction 1,
    the division 1, sqrt(q) 1, sb eps 1, sqrt(a_prev) and sa x0 2, sigma noise 1, the two additions 2."""
    coef, _, clamp = G.DDIM_VARIANTS[variant]
    c = G.ddim_coef(coef)
    t = G.ddim_x0_inputs(n)
    noise = t["noise"] if c["sigma"] > 0 else None
    args = (9.0, c["c_recip"], c["c_recipm1"], c["a_prev"])
    R = G.ddim_x0_step(t["x0_cond"], t["x0_uncond"], t["xt"], *args, clamp=clamp, sigma=c["sigma"], noise=noise)
    if clamp:
        u, cc = t["x0_uncond"].double(), t["x0_cond"].double()
        _clamp_shares(u + 9.0 * (cc - u), clamp)
    xt = t["xt"].cuda()
    ops.ddim_x0_step(t["x0_cond"].cuda(), t["x0_uncond"].cuda(), xt, *args, clamp=clamp or None, sigma=c["sigma"], noise=noise.cuda() if noise is not None else None)
    report(f"ddim_x0_step[{variant}-{n}]", xt, R, G.K["ddim_x0_step"])


@pytest.mark.parametrize("HW", [37, 131101], ids=["under", "past-cap"])
@pytest.mark.parametrize("branch", [0, 1])
def test_glue_lgm_x0_views(branch, HW):
    """vmv_lgm_x0_views, C = 4, F = 5, ld = 8, idx4 = (4, 0, 2, 2) (repeated, unordered); the other branch and the pad are NaN.
    k = 4: the two products 2, the subtraction 1, inv_scale 1."""
    Cc, F_, ld, idx4 = 4, 5, 8, (4, 0, 2, 2)
    assert (4 * Cc * HW > PAST) == (HW > 37)
    c = G.ddim_coef("last" if branch else "mid")
    eps = G.nan_pad(G.rnd((2 * F_ * HW, Cc), 1), ld)
    eps.view(2, F_ * HW, ld)[1 - branch] = float("nan")
    xt = G.rnd((Cc, F_, HW), 2)
    R = G.lgm_x0_views(eps, ld, branch, xt, idx4, c["c_recip"], c["c_recipm1"], 1.0 / 0.18215)
    out = torch.full((4, Cc, 1, HW), 7.0, device="cuda")
    ops.lgm_x0_views(eps.cuda(), ld, branch, xt.reshape(1, Cc, F_, 1, HW).cuda(), idx4, c["c_recip"], c["c_recipm1"], 1.0 / 0.18215, out)
    report(f"lgm_x0_views[b{branch}-{HW}]", out, R, G.K["lgm_x0_views"])


@pytest.mark.parametrize("V,HW", [(3, 37), (4, 58301)], ids=["under", "past-cap"])
def test_glue_lgm_pack_input(V, HW):
    """vmv_lgm_pack_input with `decoded` beyond [-1, 1] on both sides.  k = 3: 0.5 d + 0.5 rounds once (the product is exact), the subtraction
    of the mean 1, the division 1; the clamp is exact; the six ray channels are a copy (mag 0: bit-exact)."""
    assert (V * 9 * HW > PAST) == (HW > 37)
    dec, rays = G.rnd((V, 3, HW), 1, 1.2), G.rnd((V, 6, HW), 2)
    assert float((dec < -1).float().mean()) > 0.1 and float((dec > 1).float().mean()) > 0.1
    R = G.lgm_pack_input(dec, rays)
    out = torch.full((V, 9, 1, HW), 7.0, device="cuda")
    ops.lgm_pack_input(dec.reshape(V, 3, 1, HW).cuda(), rays.cuda(), out)
    report(f"lgm_pack_input[{V}x{HW}]", out, R, G.K["lgm_pack_input"])


# ------------------------------------------------------------------------------------------------- posterior, embeddings
@pytest.mark.parametrize("n,zc,HW,ld", [(2, 4, 37, 12), (2, 4, 262181, 12)], ids=["under", "past-cap"])
def test_glue_posterior_sample(n, zc, HW, ld):
    """vmv_posterior_sample, moments rows of stride 12 (NaN pad), logvar below -30, above 20 and across.  k = 3: exp() noise 1, the addition
    1, the scale 1 (0.5 logvar is exact); the exponential's (1 + |0.5 logvar| log2 e) units ride in `extra`."""
    assert (n * zc * HW > PAST) == (HW > 37)
    t = G.posterior_inputs(n, zc, HW, ld)
    lv = t["moments_rows"][:, zc:2 * zc]
    assert bool((lv < -30).any()) and bool((lv > 20).any()) and float(((lv > -30) & (lv < 20)).float().mean()) > 0.5
    R = G.posterior_sample(t["moments_rows"], ld, t["noise"], n, zc, HW, 0.18215)
    z = torch.full((n, zc, 1, HW), 7.0, device="cuda")
    ops.posterior_sample(t["moments_rows"].cuda(), ld, t["noise"].cuda(), z, 0.18215)
    report(f"posterior_sample[{HW}]", z, R, G.K["posterior_sample"])


@pytest.mark.parametrize("rows,Cc,rpt,cam_rows", [(37, 40, 5, 5), (37, 40, 5, 0), (6554, 320, 1000, 24)], ids=["under", "under-nocam", "past-cap"])
def test_glue_emb_combine_silu(rows, Cc, rpt, cam_rows):
    """vmv_emb_combine_silu with and without `cam`; cam_rows < rows, rows_per_t leaves a ragged last group.  16-bit output.  k = 6: temb + cam 1
    (and silu's slope <= 1.1 on it: 2), 1 + exp 1, the hardware reciprocal 2, the product 1; the exponential rides in `extra`."""
    assert (rows * Cc > PAST) == (rows > 37) and rows % rpt != 0
    temb = G.rnd((-(-rows // rpt), Cc), 1, 2.0)
    cam = G.rnd((cam_rows, Cc), 2, 2.0) if cam_rows else None
    R = G.emb_combine_silu(temb, cam, rows, Cc, rpt, cam_rows)
    out = torch.zeros(rows, Cc, dtype=BF, device="cuda")
    ops.emb_combine_silu(temb.cuda(), cam.cuda() if cam is not None else None, out, rows, Cc, rpt, cam_rows)
    report(f"emb_combine_silu[{rows}x{Cc}{'' if cam_rows else '-nocam'}]", out, R, G.K["emb_combine_silu"], out16=True)


@pytest.mark.parametrize("dim", [320, 37])
def test_glue_sinusoidal(dim):
    """vmv_sinusoidal at t in {0, 1, 981, 999}; an odd dim's last column is 0.  16-bit output.  k = 16 on mag = |angle| + |value|: the angle
    t 10000^(-k / half) carries the division 1, powf 4, powf's sensitivity to its rounded exponent ln(10000) = 9.2 -> 10, the product 1 — a
    relative error of the angle, an absolute one of the sine — and sinf / cosf 4 on the value."""
    t = torch.tensor([0.0, 1.0, 981.0, 999.0])
    R = G.sinusoidal(t, dim)
    out = torch.full((4, dim), 7.0, dtype=BF, device="cuda")
    ops.sinusoidal(t.cuda(), out, 4, dim)
    report(f"sinusoidal[{dim}]", out, R, G.K["sinusoidal"], out16=True)
    if dim % 2:
        assert bool((out[:, -1] == 0).all())


# ------------------------------------------------------------------------------------------------- I2VGen front end
@pytest.mark.parametrize("F_,big", [(1, False), (24, False), (64, False), (24, True), (64, True)], ids=["F1", "F24", "F64", "F24-big", "F64-big"])
def test_glue_i2v_temporal_adapter(F_, big):
    """vmv_i2v_temporal_adapter, HW = 11 (the last block of 4 pixels is ragged), nrep = 2, written at channel offset 4 of 8-wide rows; `big`:
    scores of about +-55, where the online softmax rescales by tens between keys.  16-bit output; the fp32 part of the bound is glue_ref's
    first-order error propagation through the whole chain (units(0): LayerNorm, the three linears, softmax, GELU fit), derived there stage by
    stage: a median of 0.2 to 1.8 fp16 half-ulps on top of the storage half-ulp, the big-score cases included."""
    HW, nrep = 11, 2
    x = G.rnd((F_ * HW, 4), 1).to(BF)
    w = G.adapter_weights(big)
    R = G.i2v_temporal_adapter(x, w, F_, HW, 2.0)
    if F_ > 1:
        assert (G.i2v_temporal_adapter.score_max > 40.0) == big
    out = torch.zeros(nrep * F_ * HW, 8, dtype=BF, device="cuda")
    xd, wd = x.cuda(), w.cuda()
    ops.i2v_temporal_adapter(xd, 4, out.data_ptr() + 8, 8, wd, F_, HW, nrep, 2.0)
    torch.cuda.synchronize()
    assert bool((out[:, :4] == 0).all())
    for rep in range(nrep):
        report(f"i2v_temporal_adapter[F{F_}{'-big' if big else ''}].rep{rep}", out[rep * F_ * HW:(rep + 1) * F_ * HW, 4:], R, 0, out16=True)


@pytest.mark.parametrize("n,Cc,IH,IW,OH,OW", [(2, 32, 9, 14, 4, 4), (2, 32, 5, 5, 8, 8), (2, 32, 6, 7, 6, 7), (2, 32, 160, 216, 192, 176)],
                         ids=["down", "up", "identity", "past-cap"])
def test_glue_adaptive_avgpool_rows(n, Cc, IH, IW, OH, OW):
    """vmv_adaptive_avgpool_rows at non-integer ratios down and up, the identity, and past the cap.  16-bit in and out; a bin of N elements
    is N - 1 additions and a division: units = N mag (glue_ref: units(0)).  The identity must return its input bit for bit."""
    assert (n * OH * OW * Cc > PAST) == (OH > 8)
    x = G.rnd((n * IH * IW, Cc), 3).to(BF)
    R = G.adaptive_avgpool_rows(x, n, Cc, IH, IW, OH, OW)
    y = torch.zeros(n * OH * OW, Cc, dtype=BF, device="cuda")
    xd = x.cuda()
    ops.adaptive_avgpool_rows(xd, Cc, y, Cc, n, Cc, IH, IW, OH, OW)
    torch.cuda.synchronize()
    report(f"adaptive_avgpool_rows[{IH}x{IW}->{OH}x{OW}]", y, R, 0, out16=True)
    if (IH, IW) == (OH, OW):
        assert torch.equal(bits16(y), bits16(x))


# ------------------------------------------------------------------------------------------------- LGM head
@pytest.mark.parametrize("n,zero_rot", [(1, False), (255, False), (65536, False), (65537, False), (70001, False), (255, True), (70001, True)])
def test_glue_gaussian_activation(n, zero_rot):
    """vmv_gaussian_activation, ld = 16 with NaN in columns 14 and 15; n on both sides of the 256-block cap of the first pass (65 536); scale
    inputs on both sides of the softplus threshold, opacity inputs at +-30, optionally an all-zero rotation column (the 1e-12 floor: 0).
    Per-column units from glue_ref (units(0), derived in its docstring).  The two-pass sum is deterministic: a second launch is bit-identical."""
    raw = G.gaussian_inputs(n, zero_rot)
    R = G.gaussian_activation(raw, n)
    rawd, ws = raw.cuda(), torch.zeros(1024, device="cuda")
    out = torch.full((n, 14), 7.0, device="cuda")
    ops.gaussian_activation(rawd, 16, out, n, ws)
    report(f"gaussian_activation[{n}{'-zero-rot' if zero_rot else ''}]", out, R, 0)
    if zero_rot:
        assert bool((out[:, 8] == 0).all())
    again = torch.full((n, 14), 3.0, device="cuda")
    ops.gaussian_activation(rawd, 16, again, n, torch.full((1024,), 5.0, device="cuda"))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
