"""`not gpu`: the attention test helpers (tests/attn_ref.py) and the host side of vmv_attention.

a. the fp64 reference, written from include/vmv.h, agrees with the plan interpreter's fp32 attention on every operand layout;
b. the bound of the GPU matrix is the reference's to keep: a CPU emulation of the kernels' recipe stays within HALF of it for every
   score profile — and leaves it when fp16 subnormal P's are flushed, so the GPU cases can see what they are there to see;
c. vmv_attention_served_kernel names the expected kernel for every GPU case, the production shapes and the threshold neighbours;
d. every rejection is the same code from the query and from the launcher, with nothing launched."""
import ctypes as C

import pytest
import torch

from videomv_amd import _lib as L
from videomv_amd import ops
from tests import attn_ref as R
from tests import plan_interp as I

X = 1 << 20            # a 16-byte aligned stand-in address: nothing below dereferences it


# ------------------------------------------------------------------------------------------------- a. the reference
LAYOUT_CASES = {
    "fused_spatial": dict(layout="fused", n_outer=3, heads=2, Nq=37, Nk=37),
    "temporal_inner_hw": dict(layout="temporal", n_outer=10, heads=3, Nq=7, Nk=7, inner=5),
    "cross_kv_div": dict(layout="cross", n_outer=6, heads=2, Nq=19, Nk=77, kv_div=3),
    "gathered_kv": dict(layout="gathered", n_outer=5, heads=2, Nq=3, Nk=11, inner=5),
    "causal": dict(layout="fused", n_outer=2, heads=2, Nq=41, Nk=41, causal=True),
    "head_dim_32": dict(layout="fused", n_outer=2, heads=3, Nq=29, Nk=29, hd=32),
    "head_dim_128": dict(layout="fused", n_outer=2, heads=2, Nq=21, Nk=21, hd=128),
}


@pytest.mark.parametrize("name", list(LAYOUT_CASES))
def test_attention_reference_agrees_with_the_interpreter(name):
    """The interpreter stores its fp32 result rounded to the element type, so "fp32 against fp64 to 1e-5" is stated on what it stores:
    every stored element is the rounding of SOME value within d = 1e-5 * rms(reference) of the fp64 reference (rounding is monotonic:
    round(ref - d) <= stored <= round(ref + d)), which bounds the rel-L2 of the unrounded values by 1e-5; nearly all are round(ref)
    itself.  The layouts' own inverse (reshapes and permutes) must read the same rows as the header's address formula."""
    c = R.Case(**LAYOUT_CASES[name]).fill("random", seed=3)
    t = c.on("cpu")
    p = c.build(t)
    bufs = list(t.values())
    ref = R.reference(p, bufs)
    assert ref.shape == (c.n_outer, c.heads, c.Nq, c.hd) and ref.dtype == torch.float64
    I.attention(p)
    got = R.gather(p, "o", bufs)
    assert torch.equal(got, c.logical_out(t["o"]))
    d = 1e-5 * float(ref.pow(2).mean().sqrt())
    r16 = lambda x: x.to(c.dtype).double()
    g = got.double()
    assert bool(((r16(ref - d) <= g) & (g <= r16(ref + d))).all()), float((g - ref).abs().max())
    assert float((g == r16(ref)).double().mean()) > 0.99
    if c.hd == 128:
        assert float(ref[..., 80:].abs().max()) == 0.0


def test_attention_reference_reads_the_operands_the_layout_wrote():
    """gather() (the header's formula) returns exactly the logical tensors place() put there, per layout, kv_div included."""
    for kw in LAYOUT_CASES.values():
        c = R.Case(**kw)
        q, k, v = R.patterns("random", c.n_outer, c.Pk, c.heads, c.Nq, c.Nk, c.hd, c.scale, c.dtype, seed=5, live=c.live)
        c.place(q, k, v)
        t = c.on("cpu")
        p = c.build(t)
        bufs = list(t.values())
        assert torch.equal(R.gather(p, "q", bufs), q)
        kv_of = torch.arange(c.n_outer) // c.kv_div
        assert torch.equal(R.gather(p, "k", bufs), k[kv_of]) and torch.equal(R.gather(p, "v", bufs), v[kv_of])


def test_attention_patterns_put_the_profile_into_the_scores():
    """The bias channel does what the profiles claim, on the ROUNDED tensors: the sink key leads every query by about G, `uniform` scores
    are exactly zero, a ramp's best key sits in the last (first) tile, `one_query` moves one query of sixteen."""
    Nq, Nk, G = 32, 512, 10.0
    for dtype in (torch.float16, torch.bfloat16):
        def scores(profile):
            q, k, _ = R.patterns(profile, 1, 1, 1, Nq, Nk, 64, 0.125, dtype, G, seed=1)
            return (q.double() @ k.double().transpose(-1, -2))[0, 0] * 0.125
        s = scores("early_sink")
        assert bool((s.argmax(-1) == 0).all()) and float((s[:, 0] - s[:, 1:].max(-1).values).min()) > G - 8
        s = scores("late_sink")
        assert bool((s.argmax(-1) == Nk - 3).all())
        assert float(scores("uniform").abs().max()) == 0.0
        tiles = lambda s: s.view(Nq, Nk // 64, 64).mean(-1)
        assert bool((tiles(scores("ramp_up")).diff(dim=-1) > 0.5).all()) and bool((tiles(scores("ramp_down")).diff(dim=-1) < -0.5).all())
        s = scores("one_query")
        climbs = tiles(s)[:, -1] - tiles(s)[:, 0]
        assert bool((climbs[5::16] > G / 2).all()) and float(climbs.abs().sort().values[: Nq - 2].max()) < 1.5
        s = R.patterns("large", 1, 1, 1, Nq, Nk, 64, 0.125, dtype, 60.0, seed=1)
        s = (s[0].double() @ s[1].double().transpose(-1, -2))[0, 0] * 0.125
        assert 40 < float(s.max()) < 70 and -70 < float(s.min()) < -40


# --------------------------------------------------------------------------- b. the bound is the reference's to keep
def _profile_grid():
    for profile in R.PROFILES:
        for G in ((0.0,) if profile in ("random", "uniform") else (60.0,) if profile == "large" else (6.0, 10.0, 14.0, 18.0)):
            yield profile, G


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Nk", [512, 4096])
def test_attention_emulated_recipe_keeps_half_the_bound(Nk, dtype):
    """64-key tiles, online max, P rounded to the element type (subnormals kept), fp32 accumulation: within half of
    check(6e-3, 2e-2) x TS against the fp64 reference, for every profile and gap."""
    tol_l2, tol_max = R.bound(dtype)
    worst = (0.0, 0.0)
    for profile, G in _profile_grid():
        q, k, v = R.patterns(profile, 1, 1, 2, 32, Nk, 64, 0.125, dtype, G, seed=2)
        e_l2, e_max = R.errors(R.emulate(q, k, v, 0.125), R.attend(q, k, v, 0.125))
        worst = (max(worst[0], e_l2), max(worst[1], e_max))
        assert e_l2 < 0.5 * tol_l2 and e_max < 0.5 * tol_max, (profile, G, e_l2, e_max)
    print(f"emulation, Nk {Nk}, {dtype}: worst rel-L2 {worst[0]:.2e} / max {worst[1]:.2e} (half bound {0.5 * tol_l2:.2e} / {0.5 * tol_max:.2e})")


def test_attention_flushed_subnormal_tail_breaks_the_bound():
    """One key 10 above a tail of 4095: every tail P is below 2^-14, a subnormal fp16 operand of P.V.  Kept, the recipe holds the bound;
    flushed, the tail's mass (4095 e^-10 = 0.19 of the sink's) is lost and the same bound is broken many times over."""
    q, k, v = R.patterns("early_sink", 1, 1, 2, 32, 4096, 64, 0.125, torch.float16, 10.0, seed=2)
    ref = R.attend(q, k, v, 0.125)
    tol_l2, tol_max = R.bound(torch.float16)
    kept = R.errors(R.emulate(q, k, v, 0.125), ref)
    lost = R.errors(R.emulate(q, k, v, 0.125, flush_subnormal_p=True), ref)
    assert kept[0] < 0.5 * tol_l2 and kept[1] < 0.5 * tol_max, kept
    assert lost[0] > 10 * tol_l2 and lost[1] > tol_max, lost


# ------------------------------------------------------------------------------------------------ c. dispatch table
def _shape(n_outer, heads, Nq, Nk, kv_div=1, hd=64, causal=False):
    """Dense rows (problem, token): q / o [n_outer Nq][heads hd], k | v [kv problems Nk][2 heads hd]."""
    C_ = heads * hd
    qm, km = ops.seq_map(Nq * C_, 0, C_), ops.seq_map(Nk * 2 * C_, 0, 2 * C_)
    return ops.attn_params(X, X, X + 2 * C_, X, qm, km, km, ops.seq_map(Nq * C_, 0, C_), n_outer, heads, Nq, Nk, hd ** -0.5, kv_div=kv_div,
                           head_dim=hd, causal=causal)


# (what, n_outer, heads, Nq, Nk, kv_div, head_dim, causal) -> kernel
DISPATCH = [
    # production shapes at B F = 48 (tools/attn_bench.py, latent 24 x 40 x 64) and the 24 x 32 x 32 first level
    ("self L0 2560 h5", 48, 5, 2560, 2560, 1, 64, False, "Q256"),
    ("self L1 640 h10", 48, 10, 640, 640, 1, 64, False, "Q128"),
    ("self L2 160 h20", 48, 20, 160, 160, 1, 64, False, "Q128"),
    ("cross L0 2560x77", 48, 5, 2560, 77, 24, 64, False, "Q128"),
    ("cross L1 640x77", 48, 10, 640, 77, 24, 64, False, "Q128"),
    ("temporal L0 24", 2 * 2560, 5, 24, 24, 1, 64, False, "SHORT"),
    ("temporal L1 24", 2 * 640, 10, 24, 24, 1, 64, False, "SHORT"),
    ("self 1024 h5", 48, 5, 1024, 1024, 1, 64, False, "Q256"),
    ("cross 16x77 (4 x 4 level)", 48, 20, 16, 77, 24, 64, False, "WAVE"),
    ("text tower 77", 2, 16, 77, 77, 1, 64, True, "CAUSAL"),
    ("LGM 4096 d32", 1, 16, 4096, 4096, 1, 32, False, "D32"),
    ("image tower 257 d128", 2, 16, 257, 257, 1, 128, False, "D128"),
    # Nq, Nk = 32 / 33
    ("32x32", 4, 2, 32, 32, 1, 64, False, "SHORT"),
    ("32x33", 4, 2, 32, 33, 1, 64, False, "WAVE"),
    ("33x32", 4, 2, 33, 32, 1, 64, False, "Q128"),
    ("33x33", 4, 2, 33, 33, 1, 64, False, "Q128"),
    ("1x4096", 4, 2, 1, 4096, 1, 64, False, "WAVE"),
    # Nk = 511 / 512 at 512 blocks of 256 queries
    ("Nk 511", 64, 4, 512, 511, 1, 64, False, "Q128"),
    ("Nk 512", 64, 4, 512, 512, 1, 64, False, "Q256"),
    # 511 / 512 blocks
    ("511 blocks", 73, 7, 256, 512, 1, 64, False, "Q128"),
    ("512 blocks", 64, 8, 256, 512, 1, 64, False, "Q256"),
    ("513 blocks", 57, 9, 256, 512, 1, 64, False, "Q256"),
    # a query tail: below 2048 queries only multiples of 256 take the 256-query blocks
    ("Nq 2047 with tail", 64, 1, 2047, 512, 1, 64, False, "Q128"),
    ("Nq 2048", 64, 1, 2048, 512, 1, 64, False, "Q256"),
    ("Nq 2049 with tail", 64, 1, 2049, 512, 1, 64, False, "Q256"),
    ("Nq 1280 = 5 x 256", 32, 4, 1280, 512, 1, 64, False, "Q256"),
    ("Nq 1281 with tail", 32, 4, 1281, 512, 1, 64, False, "Q128"),
    # causal and the other head widths ignore the short / long thresholds
    ("causal 17", 2, 2, 17, 17, 1, 64, True, "CAUSAL"),
    ("causal 512 x 512 blocks", 64, 4, 512, 512, 1, 64, True, "CAUSAL"),
    ("d32 short", 2, 3, 17, 17, 1, 32, False, "D32"),
    ("d128 long", 64, 4, 512, 512, 1, 128, False, "D128"),
    ("head_dim 0 = 64", 4, 2, 32, 32, 1, 0, False, "SHORT"),
]


def test_attention_dispatch_table():
    lib = L.load()
    seen = set()
    for what, n_outer, heads, Nq, Nk, kv_div, hd, causal, want in DISPATCH:
        p = _shape(n_outer, heads, Nq, Nk, kv_div, hd or 64, causal)
        p.head_dim = hd
        assert lib.vmv_attention_served_kernel(C.byref(p)) == R.branch_id(want), (what, want)
        seen.add(want)
    for name, want, *_ in R.GPU_CASES:                                   # every shape of the GPU matrix runs the kernel it names
        assert lib.vmv_attention_served_kernel(C.byref(R.params_only(name))) == R.branch_id(want), (name, want)
        seen.add(want)
    ids = {n: getattr(L, "ATTN_" + n) for n in ("SHORT", "WAVE", "Q128", "Q256", "CAUSAL", "D32", "D128")}
    assert seen == set(ids) and sorted(ids.values()) == list(range(1, 8))
    for branch in ids:                                                   # (and each branch of the GPU matrix is there at all)
        assert any(c[1] == branch for c in R.GPU_CASES), branch
    assert sum(c[1] == "Q256" for c in R.GPU_CASES) >= 4 and sum(c[1] == "WAVE" for c in R.GPU_CASES) >= 4


def test_attention_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vmv.h")).read()
    consts = dict(re.findall(r"#define\s+VMV_ATTN_([A-Z0-9]+)\s+(\d+)", hdr))
    assert len(consts) == 7
    for name, val in consts.items():
        assert getattr(L, "ATTN_" + name) == int(val), name


# --------------------------------------------------------------------------------------------------- d. rejections
ENULL, EINVAL, EALIGN, ERANGE = -3, -1, -2, -4


def _set(path, val):
    def f(p):
        obj = p
        *head, last = path.split(".")
        for a in head:
            obj = getattr(obj, a)
        setattr(obj, last, val)
    return f


def _span(rows, ok):
    """The largest accepted / smallest rejected row stride (a multiple of 8) for `rows` + 1 padded rows of 64 channels."""
    most = ((1 << 30) - 64 - 1) // rows // 8 * 8
    assert rows * most + 64 < (1 << 30) <= rows * (most + 8) + 64
    return most if ok else most + 8


REJECTIONS = [
    ("q null", _set("q", None), ENULL), ("k null", _set("k", None), ENULL), ("v null", _set("v", None), ENULL), ("o null", _set("o", None), ENULL),
    ("n_outer 0", _set("n_outer", 0), EINVAL), ("heads 0", _set("heads", 0), EINVAL), ("Nq 0", _set("Nq", 0), EINVAL), ("Nk 0", _set("Nk", 0), EINVAL),
    ("Nk < 0", _set("Nk", -5), EINVAL), ("kv_div 0", _set("kv_div", 0), EINVAL),
    ("head_dim 48", _set("head_dim", 48), EINVAL),
    ("causal, Nq != Nk", lambda p: (_set("causal", 1)(p), _set("Nk", 99)(p)), EINVAL),
    ("q s_row 68", _set("qm.s_row", 68), EALIGN), ("k s_row 132", _set("km.s_row", 132), EALIGN), ("v s_row 66", _set("vm.s_row", 66), EALIGN),
    ("o s_row 130", _set("om.s_row", 130), EALIGN), ("q s_outer 4", _set("qm.s_outer", 4), EALIGN), ("k inner 0", _set("km.inner", 0), EALIGN),
    ("q pointer + 8", _set("q", X + 8), EALIGN), ("k pointer + 2", _set("k", X + 2), EALIGN), ("o pointer + 4", _set("o", X + 4), EALIGN),
    ("q s_row < 0", _set("qm.s_row", -128), ERANGE), ("o s_row < 0", _set("om.s_row", -128), ERANGE), ("v s_row < 0", _set("vm.s_row", -256), ERANGE),
    # 100 queries pad to 256 rows, 100 keys to 128: (padded rows - 1) * s_row + head_dim must stay below 2^30 elements
    ("q span", _set("qm.s_row", _span(255, False)), ERANGE), ("o span", _set("om.s_row", _span(255, False)), ERANGE),
    ("k span", _set("km.s_row", _span(127, False)), ERANGE), ("v span", _set("vm.s_row", _span(127, False)), ERANGE),
    ("n_outer 65536, four waves", _set("n_outer", 65536), ERANGE), ("heads 65536, four waves", _set("heads", 65536), ERANGE),
]


def test_attention_rejections_agree_between_query_and_launcher():
    lib = L.load()
    ok = _shape(4, 2, 100, 100)
    assert lib.vmv_attention_served_kernel(C.byref(ok)) == L.ATTN_Q128           # (valid: never handed to the launcher here — it would launch)
    for what, spoil, code in REJECTIONS:
        p = _shape(4, 2, 100, 100)
        spoil(p)
        assert lib.vmv_attention_served_kernel(C.byref(p)) == code, what
        assert lib.vmv_attention(C.byref(p), None) == code, what
    for hd in (32, 128):                                                         # causal is the head_dim-64 kernel's; the wide grids hold for 32 / 128 too
        p = _shape(4, 2, 100, 100, hd=hd, causal=True)
        assert lib.vmv_attention_served_kernel(C.byref(p)) == lib.vmv_attention(C.byref(p), None) == EINVAL
        p = _shape(65536, 2, 100, 100, hd=hd)
        assert lib.vmv_attention_served_kernel(C.byref(p)) == lib.vmv_attention(C.byref(p), None) == ERANGE
    assert lib.vmv_attention_served_kernel(None) == lib.vmv_attention(None, None) == ENULL
    # the largest strides still accepted, one step (8 elements) below the rejected ones
    for field, rows in (("qm", 255), ("om", 255), ("km", 127), ("vm", 127)):
        p = _shape(4, 2, 100, 100)
        getattr(p, field).s_row = _span(rows, True)
        assert lib.vmv_attention_served_kernel(C.byref(p)) == L.ATTN_Q128, field
    # one wave per problem: the grid is one-dimensional, so 65536 problems per head are fine on SHORT and WAVE
    assert lib.vmv_attention_served_kernel(C.byref(_shape(65536, 2, 24, 24))) == L.ATTN_SHORT
    assert lib.vmv_attention_served_kernel(C.byref(_shape(65536, 2, 24, 77))) == L.ATTN_WAVE
    assert lib.vmv_attention_served_kernel(C.byref(_shape(65535, 2, 100, 100))) == L.ATTN_Q128
