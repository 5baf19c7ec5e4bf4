"""TEST INFRASTRUCTURE for vmv_attention: an fp64 reference, score-pattern inputs, operand layouts and a tile-wise emulation.

`reference(p, bufs)` is written from include/vmv.h alone: softmax(scale * Q K^T [causal mask]) V per (problem, head) in fp64, every
operand row fetched from the 16-bit buffers by the header's row-address formula

    base + (o / inner) * s_outer + (o % inner) * s_inner + i * s_row + h * head_dim        (elements; K / V: o -> o / kv_div)

It does not call tests/plan_interp.py (tests/test_attention_cpu.py compares the two).  The LAYOUTS below place the logical
[problem][head][row][channel] tensors into those buffers with torch reshapes and permutes only, never with that formula, so a
slip in either side shows as a disagreement.  Runs on the device of the buffers (fp64 on the GPU for the large cases).

`patterns` builds q | k | v for a wanted score profile through a BIAS CHANNEL: q[i, 0] = c_i, k[j, 0] = t_j / scale, the other
channels N(0, 1) — key j then adds exactly c_i * t_j to query i's scaled score on top of an N(0, ~1) background.  Everything is
rounded to the element type before anyone reads it, so the rounding of t costs nothing.

`emulate` follows the kernel's recipe (csrc/attention.hip) on the CPU: 64-key tiles, running max on the raw scores,
P = exp2(fma(s, sc, -m sc)) summed in fp32 but rounded to the element type for P.V, fp32 accumulation, one division at the end.
"""
import torch

from videomv_amd import _lib as L
from videomv_amd import ops

LOG2E = 1.44269504088896341
NEG_BIG = -1.0e30

# the project's attention bound (tests/test_kernels_gpu.py: check(tol_l2=6e-3, tol_max=2e-2) x TS)
TOL_L2, TOL_MAX = 6e-3, 2e-2


def ts(dtype):
    """fp16 carries three more significand bits than bf16: the bf16 bound tightened 8x."""
    return 1.0 if dtype == torch.bfloat16 else 0.125


def bound(dtype):
    return TOL_L2 * ts(dtype), TOL_MAX * ts(dtype)


def errors(out, ref):
    """(rel-L2, max-abs error / max |ref|) of `out` against the fp64 `ref` — the two figures of the project's bound."""
    a, b = out.double(), ref.double()
    assert bool(torch.isfinite(a).all()), "non-finite output"
    scale = float(b.abs().max().clamp_min(1e-6))
    return float((a - b).norm() / b.norm().clamp_min(1e-12)), float((a - b).abs().max()) / scale


# --------------------------------------------------------------------------------------------------------- reference
def _locate(ptr, bufs):
    """(flat view, element offset) of the buffer of `bufs` that holds address ptr."""
    for b in bufs:
        lo = b.data_ptr()
        if lo <= ptr < lo + b.numel() * b.element_size():
            assert (ptr - lo) % b.element_size() == 0
            return b.reshape(-1), (ptr - lo) // b.element_size()
    raise ValueError(f"address {ptr:#x} is in none of the given buffers")


def _index(m, probs, heads, n, hd, off):
    """Element index [problem][head][row][channel] of the header's row-address formula."""
    dev = probs.device
    base = torch.div(probs, m.inner, rounding_mode="floor") * m.s_outer + (probs % m.inner) * m.s_inner
    return (off + base[:, None, None, None] + torch.arange(heads, device=dev)[None, :, None, None] * hd
            + torch.arange(n, device=dev)[None, None, :, None] * m.s_row + torch.arange(hd, device=dev)[None, None, None, :])


def gather(p, which, bufs, lo=0, hi=None):
    """Rows of operand `which` ('q' | 'k' | 'v' | 'o') of problems [lo, hi) as [problem][head][row][channel], in the buffer's dtype."""
    hi = p.n_outer if hi is None else hi
    hd = p.head_dim or 64
    flat, off = _locate(getattr(p, which), bufs)
    probs = torch.arange(lo, hi, device=flat.device)
    if which in "kv":
        probs = torch.div(probs, p.kv_div, rounding_mode="floor")
    n = p.Nq if which in "qo" else p.Nk
    return flat[_index(getattr(p, which + "m"), probs, p.heads, n, hd, off)]


def attend(q, k, v, scale, causal=False):
    """fp64 softmax(scale * q k^T [key <= query]) v over the last two dimensions."""
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * float(scale)
    if causal:
        i = torch.arange(s.shape[-2], device=s.device)[:, None]
        j = torch.arange(s.shape[-1], device=s.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v.double())


def reference(p, bufs, chunk_scores=1 << 25):
    """fp64 attention of EVERY problem of *p, [n_outer][heads][Nq][head_dim], on the device of the buffers."""
    step = max(1, chunk_scores // (p.heads * p.Nq * p.Nk))
    out = []
    for lo in range(0, p.n_outer, step):
        hi = min(p.n_outer, lo + step)
        out.append(attend(gather(p, "q", bufs, lo, hi), gather(p, "k", bufs, lo, hi), gather(p, "v", bufs, lo, hi), p.scale, bool(p.causal)))
    return torch.cat(out)


# ---------------------------------------------------------------------------------------------------------- patterns
PROFILES = ("random", "uniform", "early_sink", "late_sink", "ramp_up", "ramp_down", "one_query", "large")
SINKS = ("early_sink", "late_sink", "uniform")          # V from U[1, 2): a lost tail moves the output instead of averaging to zero


def bias(profile, Nq, Nk, G, gen):
    """(c [Nq], t [Nk]) of the bias channel: key j adds c_i * t_j to query i's scaled score.  None for `random`."""
    j = torch.arange(Nk, dtype=torch.float64)
    c = torch.ones(Nq, dtype=torch.float64)
    if profile == "random":
        return None
    if profile == "uniform":
        return torch.zeros(Nq, dtype=torch.float64), torch.zeros(Nk, dtype=torch.float64)
    if profile == "early_sink":
        return c, G * (j == 0)
    if profile == "late_sink":
        return c, G * (j == max(Nk - 3, 0))
    if profile == "ramp_up":
        return c, G * j / Nk
    if profile == "ramp_down":
        return c, G * (1 - j / Nk)
    if profile == "one_query":            # one query of each 16-query group (a lane group of the kernels) climbs, fifteen do not
        return (torch.arange(Nq) % 16 == 5).double(), G * j / Nk
    if profile == "large":                # scores span +-G
        return torch.rand(Nq, generator=gen, dtype=torch.float64) * 2 - 1, G * (torch.rand(Nk, generator=gen, dtype=torch.float64) * 2 - 1)
    raise ValueError(profile)


def patterns(profile, Pq, Pk, heads, Nq, Nk, hd, scale, dtype, G=0.0, seed=0, live=None):
    """Logical q [Pq][heads][Nq][hd], k | v [Pk][heads][Nk][hd] in `dtype` for a score profile; channels >= live (default hd) are zero."""
    gen = torch.Generator().manual_seed(seed)
    live = hd if live is None else live
    q = torch.randn(Pq, heads, Nq, hd, generator=gen)
    k = torch.randn(Pk, heads, Nk, hd, generator=gen)
    v = torch.rand(Pk, heads, Nk, hd, generator=gen) + 1.0 if profile in SINKS else torch.randn(Pk, heads, Nk, hd, generator=gen)
    ct = bias(profile, Nq, Nk, G, gen)
    if profile == "uniform":
        q.zero_()
    elif ct is not None:
        q[..., 0] = ct[0].float()[None, None, :]
        k[..., 0] = (ct[1] / scale).float()[None, None, :]
    for t in (q, k, v):
        t[..., live:] = 0
    return q.to(dtype), k.to(dtype), v.to(dtype)


# ----------------------------------------------------------------------------------------------------------- layouts
class Case:
    """The operand buffers of one vmv_attention call (CPU tensors) and the argument block over a copy of them on any device."""

    def __init__(self, layout, n_outer, heads, Nq, Nk, kv_div=1, hd=64, causal=False, inner=1, dtype=None):
        assert layout in ("fused", "temporal", "cross", "gathered")
        assert layout == "cross" or kv_div == 1
        assert layout in ("cross", "gathered") or Nq == Nk
        assert layout not in ("temporal", "gathered") or n_outer % inner == 0
        self.layout, self.n_outer, self.heads, self.Nq, self.Nk, self.kv_div, self.hd, self.causal, self.inner = \
            layout, n_outer, heads, Nq, Nk, kv_div, hd, causal, inner
        self.dtype = L.elem() if dtype is None else dtype
        self.live = 80 if hd == 128 else hd           # head_dim 128 = the 80-wide heads of the CLIP image tower, zero-padded
        self.scale = self.live ** -0.5
        self.Pk = (n_outer + kv_div - 1) // kv_div
        self.t = {}

    def fill(self, profile="random", G=0.0, seed=0):
        q, k, v = patterns(profile, self.n_outer, self.Pk, self.heads, self.Nq, self.Nk, self.hd, self.scale, self.dtype, G, seed, self.live)
        return self.place(q, k, v)

    def place(self, q, k, v):
        """Logical [problem][head][row][channel] tensors -> the buffers of the layout, by reshapes and permutes only."""
        P, H, Nq, Nk, D, n = self.n_outer, self.heads, self.Nq, self.Nk, self.hd, self.inner
        C_ = H * D
        if self.layout == "fused":                 # rows (problem, token) of q | k | v
            self.t = dict(qkv=torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(P * Nq, 3 * C_))
        elif self.layout == "temporal":            # rows (batch, frame, pixel) of q | k | v; problem = (batch, pixel), inner = pixels
            s = torch.stack([q, k, v]).view(3, P // n, n, H, Nq, D)
            self.t = dict(qkv=s.permute(1, 4, 2, 0, 3, 5).reshape(P * Nq, 3 * C_))
        elif self.layout == "cross":               # q rows (problem, token); k | v rows (kv problem, token), shared by kv_div problems
            self.t = dict(q=q.permute(0, 2, 1, 3).reshape(P * Nq, C_), kv=torch.stack([k, v]).permute(1, 3, 0, 2, 4).reshape(self.Pk * Nk, 2 * C_))
        else:                                      # gathered: q in the q | k | v rows (frame, pixel) of Nq local frames, k | v in
            filler = torch.full_like(q, float("nan"))          # rows (frame, pixel) of Nk gathered frames; problem = pixel; distinct strides
            self.t = dict(qkv=torch.stack([q, filler, filler]).permute(3, 1, 0, 2, 4).reshape(Nq * P, 3 * C_),
                          kv=torch.stack([k, v]).permute(3, 1, 0, 2, 4).reshape(Nk * P, 2 * C_))
        self.t = {name: b.contiguous() for name, b in self.t.items()}
        self.t["o"] = torch.zeros(P * Nq, C_, dtype=self.dtype)
        return self

    def on(self, dev):
        return {name: b.clone().to(dev) for name, b in self.t.items()}

    def build(self, t):
        H, Nq, Nk, D, n, es = self.heads, self.Nq, self.Nk, self.hd, self.inner, 2
        C_ = H * D
        kw = dict(kv_div=self.kv_div, head_dim=D, causal=self.causal)
        if self.layout == "fused":
            m = lambda ld: ops.seq_map(Nq * ld, 0, ld, inner=1)
            b = t["qkv"].data_ptr()
            return ops.attn_params(b, b + es * C_, b + 2 * es * C_, t["o"], m(3 * C_), m(3 * C_), m(3 * C_), m(C_), self.n_outer, H, Nq, Nk, self.scale, **kw)
        if self.layout == "temporal":
            m = lambda ld: ops.seq_map(Nq * n * ld, ld, n * ld, inner=n)
            b = t["qkv"].data_ptr()
            return ops.attn_params(b, b + es * C_, b + 2 * es * C_, t["o"], m(3 * C_), m(3 * C_), m(3 * C_), m(C_), self.n_outer, H, Nq, Nk, self.scale, **kw)
        if self.layout == "cross":
            qm, km = ops.seq_map(Nq * C_, 0, C_, inner=1), ops.seq_map(Nk * 2 * C_, 0, 2 * C_, inner=1)
            kv = t["kv"].data_ptr()
            return ops.attn_params(t["q"], kv, kv + es * C_, t["o"], qm, km, km, ops.seq_map(Nq * C_, 0, C_, inner=1), self.n_outer, H, Nq, Nk, self.scale, **kw)
        P = self.n_outer
        qm, km = ops.seq_map(0, 3 * C_, P * 3 * C_, inner=P), ops.seq_map(0, 2 * C_, P * 2 * C_, inner=P)
        kv = t["kv"].data_ptr()
        return ops.attn_params(t["qkv"], kv, kv + es * C_, t["o"], qm, km, km, ops.seq_map(0, C_, P * C_, inner=P), P, H, Nq, Nk, self.scale, **kw)

    def logical_out(self, o):
        """The output buffer as [problem][head][row][channel], by reshapes and permutes only (the inverse of place())."""
        P, H, Nq, D, n = self.n_outer, self.heads, self.Nq, self.hd, self.inner
        if self.layout in ("fused", "cross"):
            return o.view(P, Nq, H, D).permute(0, 2, 1, 3)
        if self.layout == "temporal":
            return o.view(P // n, Nq, n, H, D).permute(0, 2, 3, 1, 4).reshape(P, H, Nq, D)
        return o.view(Nq, P, H, D).permute(1, 2, 0, 3)


# --------------------------------------------------------------------------------------------------------- emulation
def emulate(q, k, v, scale, flush_subnormal_p=False):
    """The kernels' recipe on [..., N, hd] tensors of the element type: 64-key tiles, online max, P rounded to the element type (an fp16 P
    below 2^-14 is a subnormal operand: kept, or flushed to zero with flush_subnormal_p), fp32 sums, one division and rounding."""
    dtype = q.dtype
    qf, kf, vf = q.float(), k.float(), v.float()
    sc = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    Nq, Nk = q.shape[-2], k.shape[-2]
    m = torch.full(q.shape[:-1], NEG_BIG, dtype=torch.float32)
    l = torch.zeros(q.shape[:-1], dtype=torch.float32)
    acc = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=torch.float32)
    for k0 in range(0, Nk, 64):
        s = torch.matmul(qf, kf[..., k0:k0 + 64, :].transpose(-1, -2))          # exact products, fp32 sums (the MFMA)
        m_new = torch.maximum(m, s.max(dim=-1).values)
        pr = torch.exp2(s * sc + (-m_new * sc)[..., None])
        alpha = torch.exp2((m - m_new) * sc)
        l = l * alpha + pr.sum(dim=-1)
        p16 = pr.to(dtype)
        if flush_subnormal_p and dtype == torch.float16:
            p16 = torch.where(p16.float() < 2.0 ** -14, torch.zeros_like(p16), p16)
        acc = acc * alpha[..., None] + torch.matmul(p16.float(), vf[..., k0:k0 + 64, :])
        m = m_new
    return (acc * (1.0 / l)[..., None]).to(dtype)


# ------------------------------------------------------------------------------------------------------ the GPU matrix
# (name, VMV_ATTN_* branch, layout, n_outer, heads, Nq, Nk, kv_div, head_dim, causal, inner) — the shapes tests/test_attention_gpu.py runs;
# tests/test_attention_cpu.py asserts, without a device, that each is served by the branch it names.
def _c(name, branch, layout, n_outer, heads, Nq, Nk, kv_div=1, hd=64, causal=False, inner=1):
    return (name, branch, layout, n_outer, heads, Nq, Nk, kv_div, hd, causal, inner)


GPU_CASES = [
    # SHORT: one wave per problem, <= 32 keys
    _c("short_9x1_4x4", "SHORT", "fused", 9, 1, 4, 4),
    _c("short_5x3_32x32", "SHORT", "fused", 5, 3, 32, 32),              # 15 problems: the last block has one idle wave
    _c("short_7x2_17x31", "SHORT", "cross", 7, 2, 17, 31),
    _c("short_3x1_1x32", "SHORT", "cross", 3, 1, 1, 32),
    _c("short_gathered_3x24", "SHORT", "gathered", 10, 2, 3, 24, inner=10),
    _c("short_temporal_24", "SHORT", "temporal", 12, 2, 24, 24, inner=6),
    # WAVE: one wave per problem, key tiles of 64
    _c("wave_cross_16x77", "WAVE", "cross", 6, 2, 16, 77, kv_div=3),
    _c("wave_5x3_32x64", "WAVE", "cross", 5, 3, 32, 64),                # an exact tile, 15 problems
    _c("wave_3x1_1x33", "WAVE", "cross", 3, 1, 1, 33),
    _c("wave_3x1_1x65", "WAVE", "cross", 3, 1, 1, 65),                  # one key in the second tile
    _c("wave_4x2_24x130", "WAVE", "cross", 4, 2, 24, 130),              # three tiles, partial last
    _c("wave_2x1_32x300", "WAVE", "cross", 2, 1, 32, 300),
    # Q128: four waves per 128-query block
    *[_c(f"q128_40x{nk}", "Q128", "cross", 2, 2, 40, nk) for nk in (33, 63, 64, 65, 128, 129)],
    *[_c(f"q128_{nq}x100", "Q128", "cross", 2, 2, nq, 100) for nq in (33, 127, 128, 129)],
    _c("q128_3x5_130", "Q128", "fused", 3, 5, 130, 130),                # 30 blocks, nblk & 7 = 6
    _c("q128_64x4096", "Q128", "cross", 1, 1, 64, 4096),
    _c("q128_temporal_40", "Q128", "temporal", 6, 2, 40, 40, inner=3),
    # Q256: four waves per 256-query block
    _c("q256_512", "Q256", "fused", 64, 4, 512, 512),                   # 512 blocks, nblk & 7 = 0
    _c("q256_2100x577", "Q256", "cross", 19, 3, 2100, 577, kv_div=19),  # 513 blocks; last query block 52 rows; ten key tiles, one key in the last
    _c("q256_1024", "Q256", "fused", 32, 4, 1024, 1024),                # 512 blocks: the 24 x 32 x 32 production tile walk
    _c("q256_256x513", "Q256", "cross", 172, 3, 256, 513, kv_div=4),    # 516 blocks, nblk & 7 = 4; one query block per problem
    # CAUSAL
    *[_c(f"causal_{T}", "CAUSAL", "fused", 2, 2, T, T, causal=True) for T in (1, 17, 64, 65, 129)],
    # head_dim 32 / 128
    *[_c(f"d32_{T}", "D32", "fused", 2, 3, T, T, hd=32) for T in (64, 65, 130)],
    *[_c(f"d128_{T}", "D128", "fused", 2, 2, T, T, hd=128) for T in (17, 129)],
    # Nk = 1: the output is V's row, bit for bit
    _c("short_32x1", "SHORT", "cross", 3, 2, 32, 1),
    _c("q128_100x1", "Q128", "cross", 2, 2, 100, 1),
    _c("d32_70x1", "D32", "cross", 2, 3, 70, 1, hd=32),
    _c("d128_40x1", "D128", "cross", 2, 2, 40, 1, hd=128),
]
CASE_BY_NAME = {c[0]: c for c in GPU_CASES}


def branch_id(name):
    return getattr(L, "ATTN_" + name)


def case(name, dtype=None):
    _, _, layout, n_outer, heads, Nq, Nk, kv_div, hd, causal, inner = CASE_BY_NAME[name]
    return Case(layout, n_outer, heads, Nq, Nk, kv_div=kv_div, hd=hd, causal=causal, inner=inner, dtype=dtype)


def params_only(name):
    """The argument block of a GPU case over fake addresses: what vmv_attention_served_kernel needs, and no memory."""
    c = case(name)

    class _B:
        def __init__(self, a):
            self.a = a

        def data_ptr(self):
            return self.a
    return c.build({k: _B(1 << 20) for k in ("qkv", "q", "kv", "o")})
