"""TEST INFRASTRUCTURE: float64 references of the 14 sampler / LGM glue entry points, written from the "Sampler glue", "I2VGen-XL front-end
helpers" and "Glue of the LGM-refined sampling step" blocks of include/vmv.h and the reference lines those cite.  Independent of
tests/plan_interp.py (fp32, cross-checked against this file in tests/test_glue_cpu.py) and of the kernels (tests/test_glue_gpu.py).

Inputs are the very tensors a kernel is given (fp32, or the 16-bit element type) widened to float64; scalar coefficients are widened from
their fp32 value (`f32`), because the C ABI passes `float`.  Layout functions return the moved values (float64 of the unrounded source).
Arithmetic functions return a `Ref`:

    ref     the float64 result
    mag     per element, the sum of the absolute values of the terms that meet in the result — what an fp32 evaluation can be held to
    extra   per element, error units (multiples of 2^-24, absolute) that do not scale with an operation count: the argument-dependent
            part of every exponential, the conditioning of sqrt(1 - a_prev - sigma^2), the absolute error of the erf-GELU fit

so that a fp32 kernel of k rounding operations obeys |got - ref| <= 2^-24 * (k * mag + extra).  `units(k)` is that parenthesis.
"""
import collections
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32 (half an ulp, relative)
LOG2E = 1.4426950408889634
D = torch.float64


class Ref(collections.namedtuple("Ref", "ref mag extra")):
    def units(self, k):
        return k * self.mag + self.extra


def f32(v):
    """the float64 value of a scalar after its conversion to the `float` of the C ABI"""
    return float(np.float32(v))


def d(t):
    return t.detach().cpu().to(D)


def half_ulp(ref, dtype):
    """half an ulp of the 16-bit type `dtype` at |ref| (normal range; the smallest subnormal spacing below it)"""
    bits, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.frexp(ref.abs().clamp_min(2.0 ** emin))[1].to(D) - 1
    return torch.exp2(e - bits - 1)


def check(name, got, R, k, elem=None, tag=""):
    """assert |got - ref| <= 2^-24 units(k) (+ half an ulp of the 16-bit type `elem` at ref) on EVERY element; print the measured maximum of
    |got - ref| / (2^-24 mag) first.  -> that ratio"""
    got = d(got).reshape(R.ref.shape)
    assert torch.isfinite(got).all(), name
    err = (got - R.ref).abs()
    bound = U * R.units(k) + (half_ulp(R.ref, elem) if elem is not None else 0.0)
    nz = R.mag > 0
    ratio = float((err[nz] / (U * R.mag[nz])).max()) if nz.any() else 0.0
    pos = bound > 0
    rel = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    part = ""
    if elem is not None and nz.any():          # what is left of the error beyond the storage rounding: the fp32 arithmetic's share
        part = f" beyond the half ulp={float(((err - half_ulp(R.ref, elem)).clamp_min(0.0)[nz] / (U * R.mag[nz])).max()):.3f}"
    eff = (R.units(k)[nz] / R.mag[nz]) if nz.any() else torch.zeros(1, dtype=D)          # the effective k: the fp32 part of the bound per unit of mag
    print(f"[glue] {name} {tag} k={k} effective k median={float(eff.median()):.1f} max={float(eff.max()):.1f} "
          f"max|got-ref|/(2^-24 mag)={ratio:.3f}{part} max err/bound={rel:.3f}")
    bad = err > bound
    if bad.any():
        i = int((err - bound).reshape(-1).argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst at flat index {i}: got {float(got.reshape(-1)[i])!r}, "
                             f"ref {float(R.ref.reshape(-1)[i])!r}, err {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}; "
                             f"max ratio to 2^-24 mag {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------------------------------------- layout moves
def latent_to_rows(x, Cpad, nrep):
    """x [nb][C][F][H][W] -> rows [nrep * nb * F * H * W][Cpad]: row (rep, b, f, pixel) holds the C channels, then zeros"""
    nb, Cc, F_, H, W = x.shape
    out = torch.zeros(nrep, nb, F_, H * W, Cpad, dtype=D)
    for c in range(Cc):
        out[:, :, :, :, c] = d(x)[:, c].reshape(nb, F_, H * W)[None]
    return out.reshape(nrep * nb * F_ * H * W, Cpad)


def latent_to_rows_keep(x, nrep):
    """the values of channels [0, C) of every row (the caller checks that the other columns keep their contents)"""
    return latent_to_rows(x, x.shape[1], nrep)


def rows_to_nchw(rows, n, Cc, HW):
    """rows [n * HW][ld] -> [n][C][HW]: out[i][c][p] = rows[i * HW + p][c]"""
    r = d(rows).reshape(n, HW, -1)
    out = torch.empty(n, Cc, HW, dtype=D)
    for c in range(Cc):
        out[:, c] = r[:, :, c]
    return out


# ------------------------------------------------------------------------------------------------- DDIM updates
def _ddim_tail(x0, m0, crxt, crm1, a_prev, sigma, noise, clamp):
    """x0 (its term magnitude m0) -> clamp, eps = (cr xt - x0) / crm1, sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma^2) eps + sigma noise"""
    if clamp and clamp > 0:
        x0 = x0.clamp(-clamp, clamp)
    eps = (crxt - x0) / crm1
    q = 1.0 - a_prev - sigma * sigma
    assert q >= 0.0
    sa, sb = math.sqrt(a_prev), math.sqrt(q)
    nx = sa * x0 + sb * eps
    mag = sa * m0 + sb / abs(crm1) * (crxt.abs() + m0)
    if sigma > 0:
        nx = nx + sigma * noise
        mag = mag + (sigma * noise).abs()
    # the roundings of q = 1 - a_prev - sigma^2 that actually occur: 1 - a_prev is exact for a_prev >= 0.5 (Sterbenz) and rounds by one unit of
    # its own size below; sigma^2 and the second subtraction round only when sigma > 0 (one unit of sigma^2, one of q; a fused multiply-add
    # does less).  d sqrt(q) = dq / (2 sqrt(q)); sqrt's own rounding is in k.  sigma = 0 with a_prev >= 0.5, and q == 0, leave nothing.
    dq = (1.0 - a_prev if a_prev < 0.5 else 0.0) + (sigma * sigma + q if sigma > 0 else 0.0)
    extra = eps.abs() * (dq / (2.0 * sb) if q > 0 else 0.0)
    return x0, Ref(nx, mag, extra)


def ddim_x0_step(x0_cond, x0_uncond, xt, guide, c_recip, c_recipm1, a_prev, clamp=0.0, sigma=0.0, noise=None):
    """x0 = u + guide (c - u); see _ddim_tail.  -> Ref of the new xt"""
    g, cr, crm1, ap, sg, cl = f32(guide), f32(c_recip), f32(c_recipm1), f32(a_prev), f32(sigma), f32(clamp or 0.0)
    c, u, x = d(x0_cond), d(x0_uncond), d(xt)
    x0 = u + g * (c - u)
    m0 = u.abs() + (g * c).abs() + (g * u).abs()
    return _ddim_tail(x0, m0, cr * x, crm1, ap, sg, d(noise) if noise is not None else None, cl)[1]


def cfg_ddim_step(eps_rows, ld, xt, guide_scale, c_recip, c_recipm1, c_sqrt_ac, c_sqrt_1mac, a_prev, v_pred=False, clamp=0.0, sigma=0.0,
                  noise=None):
    """eps_rows [2][F * HW][ld] (branch 0 conditional, 1 unconditional), xt [C][F][HW] -> (Ref of the new xt, Ref of x0_out)"""
    Cc, F_, HW = xt.shape
    g, cr, crm1, sac, s1m = f32(guide_scale), f32(c_recip), f32(c_recipm1), f32(c_sqrt_ac), f32(c_sqrt_1mac)
    e = d(eps_rows).reshape(2, F_ * HW, ld)
    y = torch.stack([e[0, :, c] for c in range(Cc)]).reshape(Cc, F_, HW)
    u = torch.stack([e[1, :, c] for c in range(Cc)]).reshape(Cc, F_, HW)
    x = d(xt)
    out = u + g * (y - u)
    mo = u.abs() + (g * y).abs() + (g * u).abs()
    a, b = (sac, s1m) if v_pred else (cr, crm1)
    x0 = a * x - b * out
    m0 = (a * x).abs() + abs(b) * mo
    x0c, nx = _ddim_tail(x0, m0, cr * x, crm1, f32(a_prev), f32(sigma), d(noise).reshape(Cc, F_, HW) if noise is not None else None, f32(clamp or 0.0))
    return nx, Ref(x0c, m0, torch.zeros_like(m0))


# ------------------------------------------------------------------------------------------------- VAE posterior, embeddings
def posterior_sample(moments_rows, ld, noise, n, zc, HW, scale):
    """moments rows [n * HW][ld] = (mean[zc] | logvar[zc] | ...), noise [n][zc][HW] -> z [n][zc][HW]"""
    m = d(moments_rows).reshape(n, HW, ld)
    mean = torch.stack([m[:, :, c] for c in range(zc)], dim=1)
    logvar = torch.stack([m[:, :, zc + c] for c in range(zc)], dim=1).clamp(-30.0, 20.0)
    s = f32(scale)
    en = torch.exp(0.5 * logvar) * d(noise).reshape(n, zc, HW)
    return Ref(s * (mean + en), abs(s) * (mean.abs() + en.abs()), abs(s) * en.abs() * (1.0 + (0.5 * logvar).abs() * LOG2E))


def emb_combine_silu(temb, cam, rows, Cc, rows_per_t, cam_rows):
    """e[r][c] = silu(temb[r // rows_per_t][c] + cam[r % cam_rows][c])"""
    r = torch.arange(rows)
    t = d(temb)[r // rows_per_t]
    v, mag = t, t.abs()
    if cam is not None:
        c = d(cam)[r % cam_rows]
        v, mag = t + c, t.abs() + c.abs()
    sg = 1.0 / (1.0 + torch.exp(-v))
    # exp(-v) enters the result through 1 / (1 + exp(-v)): its relative error is weighted by exp(-v) / (1 + exp(-v)) = 1 - sigmoid
    return Ref(v * sg, mag, (v * sg).abs() * (1.0 - sg) * (1.0 + v.abs() * LOG2E))


def sinusoidal(t, dim, base=10000.0):
    """[n][dim] = cos(t f_k) for k < dim // 2 || sin(t f_k), f_k = 10000^(-k / (dim // 2)); an odd dim leaves its last column 0.
    mag = |angle| + |value|: the angle's relative error (division, power, product) is an ABSOLUTE error of the angle-sized argument"""
    half = dim // 2
    ang = torch.outer(d(t), torch.pow(torch.tensor(base, dtype=D), -torch.arange(half, dtype=D) / half))
    ref = torch.zeros(t.numel(), dim, dtype=D)
    ref[:, :half], ref[:, half:2 * half] = torch.cos(ang), torch.sin(ang)
    mag = torch.zeros_like(ref)
    mag[:, :2 * half] = torch.cat([ang, ang], dim=1).abs() + ref[:, :2 * half].abs()
    return Ref(ref, mag, torch.zeros_like(ref))


# ------------------------------------------------------------------------------------------------- I2VGen front end
GELU_FIT_UNITS = 6.7e-7 / U          # the documented absolute error of the one-transcendental erf-GELU, in units


def _lin(v, e, W, b):
    """y = W v + b with a running absolute error bound (units): the incoming error through |W|, one rounding per product and per addition"""
    y = v @ W.t() + (b if b is not None else 0.0)
    mag = v.abs() @ W.abs().t() + (b.abs() if b is not None else 0.0)
    return y, e @ W.abs().t() + (W.shape[1] + 1) * mag, mag


def i2v_temporal_adapter(x, w, F_, HW, scale):
    """x: rows [F * HW][4] (frame-major), w: the 288-float parameter block -> Ref [F * HW][4] of scale * TransformerV2(x) over the F frames of
    every pixel.  A chain this long has no single operation count: `extra` carries a running first-order error bound (units) built stage by
    stage from the rules of this file (one unit per rounding, (1 + |arg| log2 e) per fast exponential, 2 per reciprocal square root), `mag`
    the terms of the last sum; use units(0)."""
    w = d(w)
    ln_g, ln_b, Wqkv, Wo, bo = w[0:4], w[4:8], w[8:104].view(24, 4), w[104:136].view(4, 8), w[136:140]
    W1, b1, W2, b2 = w[140:204].view(16, 4), w[204:220], w[220:284].view(4, 16), w[284:288]
    x = d(x).reshape(F_, HW, 4).permute(1, 0, 2)                                   # pix f c
    mean = x.mean(-1, keepdim=True)
    e_mean = 4 * x.abs().mean(-1, keepdim=True)
    dd = x - mean
    e_d = e_mean + dd.abs()
    var = (dd * dd).mean(-1, keepdim=True) + 1e-5
    e_var = (2 * dd.abs() * e_d).mean(-1, keepdim=True) + 9 * var
    rstd = var.rsqrt()
    e_rstd = 0.5 * rstd / var * e_var + 2 * rstd
    hn = dd * rstd * ln_g + ln_b
    e_hn = (e_d * rstd + dd.abs() * e_rstd) * ln_g.abs() + 3 * ((dd * rstd * ln_g).abs() + ln_b.abs())
    qkv, e_qkv, _ = _lin(hn, e_hn, Wqkv, None)
    sp = lambda t: t.reshape(HW, F_, 3, 2, 4).permute(2, 0, 3, 1, 4)               # (q|k|v) pix head f d
    (q, k, v), (eq, ek, ev) = sp(qkv), sp(e_qkv)
    s = 0.5 * q @ k.transpose(-1, -2)
    e_s = 0.5 * (eq @ k.abs().transpose(-1, -2) + q.abs() @ ek.transpose(-1, -2)) + 5 * 0.5 * (q.abs() @ k.abs().transpose(-1, -2))
    i2v_temporal_adapter.score_max = float(s.abs().max())          # (the tests assert which softmax regime a parameter block reaches)
    p = torch.softmax(s, dim=-1)
    smax, smin = s.max(-1, keepdim=True)[0], s.min(-1, keepdim=True)[0]
    o = p @ v
    # online softmax, to first order.  A relative error eta_j of weight j moves the output by p_j eta_j (v_j - o): what is common to all
    # weights cancels between the accumulator and the row sum.  eta_j = the score's own error, its exponential (|arg| <= max - s_j), and the
    # rescales exp(m_old - m_new) applied after key j (at most F, their arguments sum to at most the row's range).  What the accumulator and
    # the sum do not share are their own roundings: 3 per key on the accumulator, 2 on the sum, the division: (5 F + 1) on sum_j p_j |v_j|.
    eta = e_s + (1 + (smax - s) * LOG2E) + (F_ + (smax - smin) * LOG2E)
    dev = (v.unsqueeze(-3) - o.unsqueeze(-2)).abs()                                 # pix head i j d: |v_j - o_i|
    e_o = ((p * eta).unsqueeze(-1) * dev).sum(-2) + (5 * F_ + 1) * (p @ v.abs()) + p @ ev
    cat = lambda t: t.permute(0, 2, 1, 3).reshape(HW, F_, 8)
    y, e_y, m_y = _lin(cat(o), cat(e_o), Wo, bo)
    y, e_y, m_y = y + x, e_y + (y + x).abs(), m_y + x.abs()
    pre, e_pre, _ = _lin(y, e_y, W1, b1)
    hid = torch.nn.functional.gelu(pre)
    e_hid = 1.13 * e_pre + GELU_FIT_UNITS                                           # max |gelu'| = 1.129
    z, e_z, m_z = _lin(hid, e_hid, W2, b2)
    sc = f32(scale)
    res = sc * (z + y)
    e_res = abs(sc) * (e_z + e_y + (z + y).abs()) + res.abs()
    back = lambda t: t.permute(1, 0, 2).reshape(F_ * HW, 4)
    return Ref(back(res), back(abs(sc) * (m_z + m_y)), back(e_res))


def _bins(I, O):
    """[O][I] indicator of nn.AdaptiveAvgPool2d's bins [floor(o I / O), ceil((o + 1) I / O))"""
    m = torch.zeros(O, I, dtype=D)
    for o in range(O):
        m[o, (o * I) // O: -((-(o + 1) * I) // O)] = 1.0
    return m


def adaptive_avgpool_rows(x, n, Cc, IH, IW, OH, OW):
    """x rows [n * IH * IW][>= C] -> Ref [n * OH * OW][C]: the mean over the bin of each axis (nn.AdaptiveAvgPool2d).  A bin of N elements
    costs N - 1 additions and a division: `extra` = N * mag; use units(0)."""
    xs = d(x).reshape(n, IH, IW, -1)[..., :Cc]
    by, bx = _bins(IH, OH), _bins(IW, OW)
    cnt = (by.sum(1)[:, None] * bx.sum(1)[None, :])[None, :, :, None]
    pool = lambda t: torch.einsum("oy,nyxc,px->nopc", by, t, bx) / cnt
    sh = (n * OH * OW, Cc)
    ref, mag = pool(xs).reshape(sh), pool(xs.abs()).reshape(sh)
    return Ref(ref, mag, (cnt * pool(xs.abs())).reshape(sh))


# ------------------------------------------------------------------------------------------------- LGM glue
def lgm_x0_views(eps_rows, ld, branch, xt, idx4, c_recip, c_recipm1, inv_scale):
    """eps_rows [2 * F * HW][ld] branch-major, xt [C][F][HW] -> Ref [4][C][HW]: inv_scale (c_recip xt[:, f] - c_recipm1 eps_branch[f]), f = idx4[v]"""
    Cc, F_, HW = xt.shape
    cr, crm1, inv = f32(c_recip), f32(c_recipm1), f32(inv_scale)
    e = d(eps_rows).reshape(2, F_, HW, ld)[branch]
    x = d(xt)
    ref, mag = torch.empty(4, Cc, HW, dtype=D), torch.empty(4, Cc, HW, dtype=D)
    for v, f in enumerate(idx4):
        for c in range(Cc):
            a, b = cr * x[c, f], crm1 * e[f, :, c]
            ref[v, c], mag[v, c] = inv * (a - b), abs(inv) * (a.abs() + b.abs())
    return Ref(ref, mag, torch.zeros_like(mag))


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def lgm_pack_input(decoded, rays):
    """decoded [V][3][HW], rays [V][6][HW] -> Ref [V][9][HW]: (clamp(0.5 d + 0.5, 0, 1) - mean) / std (ImageNet, as fp32 constants) | rays.
    The ray channels are a copy: mag = 0 there (bit-exact)."""
    V, _, HW = decoded.shape
    ref, mag = torch.zeros(V, 9, HW, dtype=D), torch.zeros(V, 9, HW, dtype=D)
    for c in range(3):
        x = (d(decoded)[:, c] * 0.5 + 0.5).clamp(0.0, 1.0)
        ref[:, c] = (x - f32(IMAGENET_MEAN[c])) / f32(IMAGENET_STD[c])
        mag[:, c] = (x.abs() + f32(IMAGENET_MEAN[c])) / f32(IMAGENET_STD[c])
    ref[:, 3:9] = d(rays)
    return Ref(ref, mag, torch.zeros_like(mag))


def lgm_render_to_vae(images, S):
    """images [V][3][S_in][S_in] -> [V][3][S][S]: out[y][x] = (img[floor(y S_in / S)][floor(x S_in / S)] - 0.5) / 0.5.  One fp32 subtraction
    (the division by 0.5 is exact): the float32 rounding of this float64 value is the only correct fp32 result."""
    S_in = images.shape[-1]
    idx = (torch.arange(S) * S_in) // S
    return (d(images)[:, :, idx][:, :, :, idx] - 0.5) / 0.5


def gaussian_rot_sum_depth(n):
    """additions on the longest path of the kernel contract's "deterministic two-pass sum" of n squares: <= 256 blocks of 256 threads each
    take a strided share, a binary tree folds the block (8 levels), the partials are folded in order"""
    nparts = min(256, -(-n // 256))
    return -(-n // (256 * nparts)) + 8 + nparts


def gaussian_activation(raw, n):
    """raw rows [n][ld >= 14] -> Ref [n][14] = pos.clamp(-1, 1) | sigmoid | 0.1 softplus (threshold 20) | rotation component / max(L2 norm over
    the n rows, 1e-12) | 0.5 tanh + 0.5.  Per-column operation counts differ, so `extra` carries them; use units(0):
    pos 0 (exact); sigmoid: exp 4 weighted by 1 - sigmoid, add, divide; softplus: exp 4, log1p 4, multiply (one multiply above the threshold);
    rotation: half the depth of the sum (the square root), one per square, sqrt, divide, multiply; rgb: tanh 4 on its term, multiply, add."""
    x = d(raw)[:n, :14]
    ref, un = torch.empty(n, 14, dtype=D), torch.zeros(n, 14, dtype=D)
    ref[:, 0:3] = x[:, 0:3].clamp(-1.0, 1.0)
    sg = torch.sigmoid(x[:, 3])
    ref[:, 3], un[:, 3] = sg, sg * (4 * (1 - sg) + 2)
    sc = x[:, 4:7]
    ref[:, 4:7] = 0.1 * torch.where(sc > 20.0, sc, torch.log1p(torch.exp(sc.clamp(max=20.0))))
    un[:, 4:7] = ref[:, 4:7].abs() * torch.where(sc > 20.0, 1.0, 9.0)
    rot = x[:, 7:11]
    ref[:, 7:11] = rot / rot.norm(dim=0, keepdim=True).clamp_min(f32(1e-12))
    un[:, 7:11] = ref[:, 7:11].abs() * (0.5 * (gaussian_rot_sum_depth(n) + 1) + 3)
    th = torch.tanh(x[:, 11:14])
    ref[:, 11:14] = 0.5 * th + 0.5
    un[:, 11:14] = 4 * 0.5 * th.abs() + 2 * (0.5 * th.abs() + 0.5)
    mag = ref.abs()
    mag[:, 11:14] = 0.5 * th.abs() + 0.5
    return Ref(ref, mag, un)


# ------------------------------------------------------------------------------------------------- case inputs (shared by both test files)
# k of the kernels with one operation count (derived in the docstrings of tests/test_glue_gpu.py); the others carry their units in `extra`
K = {"cfg_ddim_step": 16, "cfg_ddim_step.x0_out": 6, "ddim_x0_step": 13, "lgm_x0_views": 4, "lgm_pack_input": 3, "posterior_sample": 3,
     "emb_combine_silu": 6, "sinusoidal": 16, "i2v_temporal_adapter": 0, "adaptive_avgpool_rows": 0, "gaussian_activation": 0}
CAP = 8192 * 256          # elements one pass of a glue kernel's grid covers (grid_for: 8192 blocks of 256 threads); beyond it the loop runs again


def g(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=g(seed)) * scale


def nan_pad(data, ld):
    """[rows][width] -> [rows][ld] fp32 with NaN in the columns a kernel must not read"""
    out = torch.full((data.shape[0], ld), float("nan"))
    out[:, :data.shape[1]] = data
    return out


def ddim_coef(variant):
    """fp32 coefficient sets from the reference's own tables (oracle/ddim_ref.DDIMTables, linear_sd, 1000 steps, stride 20):
    mid: t = 501; eta: the same with eta = 1 (sigma as the host computes it, in fp32); last: t = 1, a_prev = abar_0 — sqrt(1 / abar - 1) = 0.041,
    where eps = (cr xt - x0) / crm1 cancels; sb0: sigma^2 = 1 - a_prev exactly (0.25), so the direction term vanishes"""
    from oracle.ddim_ref import DDIMTables, betas_for
    tb = DDIMTables(betas_for("linear_sd"))
    t = 1 if variant == "last" else 501
    a_t, a_prev = np.float32(tb.ac[t]), np.float32(tb.ac[max(t - 20, 0)])
    c = dict(c_recip=float(np.float32(tb.sqrt_recip[t])), c_recipm1=float(np.float32(tb.sqrt_recipm1[t])), c_sqrt_ac=float(np.float32(tb.sqrt_ac[t])),
             c_sqrt_1mac=float(np.float32(tb.sqrt_1mac[t])), a_prev=float(a_prev), sigma=0.0)
    if variant == "eta":
        c["sigma"] = float(np.sqrt((np.float32(1) - a_prev) / (np.float32(1) - a_t) * (np.float32(1) - a_t / a_prev), dtype=np.float32))
    if variant == "sb0":
        c.update(a_prev=0.75, sigma=0.5)
    return c


# cfg_ddim_step / ddim_x0_step variants: (coefficients, v_pred, clamp)
DDIM_VARIANTS = {"eps": ("mid", False, 0.0), "v": ("mid", True, 0.0), "eps-clamp": ("mid", False, 1.0), "v-clamp-eta": ("eta", True, 0.7), "eps-eta": ("eta", False, 0.0),
                 "eps-sb0": ("sb0", False, 0.0), "eps-last": ("last", False, 0.0), "eps-last-clamp": ("last", False, 1.0)}


def cfg_ddim_inputs(Cc, F_, HW, ld, seed=1):
    """the two branches' predictions differ by a tenth of their size, as the conditional and unconditional outputs of one model do"""
    e = rnd((F_ * HW, Cc), seed)
    return dict(eps_rows=nan_pad(torch.cat([e + 0.1 * rnd((F_ * HW, Cc), seed + 3), e]), ld), xt=rnd((Cc, F_, HW), seed + 1), noise=rnd((Cc, F_, HW), seed + 2))


def ddim_x0_inputs(n, seed=1):
    u = rnd((n,), seed)
    return dict(x0_cond=u + 0.3 * rnd((n,), seed + 1), x0_uncond=u, xt=rnd((n,), seed + 2), noise=rnd((n,), seed + 3))


def posterior_inputs(n, zc, HW, ld, seed=1):
    """logvar = 15 N(0, 1) - 5: about 5 % below -30, 5 % above 20, the rest across the interval"""
    mom = torch.cat([rnd((n * HW, zc), seed), 15.0 * rnd((n * HW, zc), seed + 1) - 5.0], dim=1)
    return dict(moments_rows=nan_pad(mom, ld), noise=rnd((n, zc, HW), seed + 2))


def gaussian_inputs(n, zero_rot=False, seed=11):
    """raw [n][16], NaN in columns 14 and 15; scale inputs on both sides of the softplus threshold, opacity inputs at +-30"""
    raw = nan_pad(2.0 * rnd((n, 14), seed), 16)
    raw[0::5, 4], raw[1::5, 5], raw[2::5, 6], raw[3::5, 4], raw[3::5, 3], raw[4::5, 3] = 19.9, 20.1, 25.0, -25.0, 30.0, -30.0
    if n > 1:
        raw[0, 4], raw[1, 4] = 20.0, float(np.nextafter(np.float32(20.0), np.float32(21.0)))
    if zero_rot:
        raw[:, 8] = 0.0
    return raw


def adapter_weights(big_scores=False, seed=2):
    """the 288-float parameter block; big_scores: the q and k rows of Wqkv scaled by 4, so that the scores q.k / 2 reach about +-55 and the
    running maximum of the online softmax moves by tens between keys"""
    w = 0.5 * rnd((288,), seed)
    w[0:4] = 1 + 0.1 * w[0:4]
    if big_scores:
        w[8:8 + 64] *= 4.0
    return w
