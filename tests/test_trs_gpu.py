"""The row-stationary temporal convolution (csrc/gemm_trs.hip, VMV_TILE_TRS) on the GPU — `pytest -m gpu`.

Reference: fp64 on the host from the 16-bit inputs — the norm applied from the SAME table the kernel reads (vmv_groupnorm_table's
output), rounded to the 16-bit element type as the kernel rounds it, then Conv3d (3,1,1) with zero padding, bias, residual.
Tolerance: for every random-data case the rel-L2 error against fp64 of (a) the new kernel and (b) the path it replaces on the same
inputs (vmv_groupnorm_apply + VMV_TILE_X256x320; the library's own policy where that tile does not serve the shape) is computed and
printed, and (a) <= 1.5 x (b) is required: both multiply the same 16-bit operands and round the same fp32 sums to 16 bits, the only
difference is the fp32 summation order of the three taps, so the factor is slack for that and not for a bug.  Impulse cases and the
folded-vs-two-launch comparison are exact.

Measured (MI355X, fp16 / bf16 child): see DESIGN.md §5.1.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from videomv_amd import _lib as L
from videomv_amd import ops, packing as P

pytestmark = pytest.mark.gpu
BF = L.elem()
CC = 320
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 77.0          # sentinel of the pad columns of a padded output (exact in fp16 and bf16)


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2_64(a, ref):
    a, ref = a.double().cpu(), ref.double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def conv_ref64(xn, wt16, bias, res, Bn, F_, Pp, N):
    """Conv3d (3,1,1), zero padding, in fp64: xn [M][C] 16-bit rows (b, f, p), wt16 [N][C][3][1][1] 16-bit."""
    x5 = xn.double().view(Bn, F_, Pp, CC).permute(0, 3, 1, 2)[..., None]
    y = torch.nn.functional.conv3d(x5, wt16.double(), None if bias is None else bias.double(), padding=(1, 0, 0))
    y = y[..., 0].permute(0, 2, 3, 1).reshape(Bn * F_ * Pp, N)
    return y if res is None else y + res.double()


def fold_ref(x, tab, rps, silu):
    """elem(silu(x * scale + shift)) with the table's values: fp32 value of the fused multiply-add (exact product in fp64), SiLU,
    one rounding to the 16-bit type"""
    M = x.shape[0]
    t = tab.view(-1, 2, CC).double()
    s = torch.arange(M) // rps
    v = (x.double() * t[s, 0] + t[s, 1]).float().double()
    if silu:
        v = v * torch.sigmoid(v)
    return v.float().to(BF)


class Tc:
    """One case on the device: operands, the real statistics -> table pipeline, launches of the new kernel and of the old path."""

    def __init__(self, Bn, F_, Pp, N, bias=True, res=False, pad=False, seed=1):
        self.Bn, self.F, self.P, self.N = Bn, F_, Pp, N
        self.M, self.rps = Bn * F_ * Pp, F_ * Pp
        M = self.M
        self.wt = (torch.randn(N, CC, 3, 1, 1, generator=g(seed + 1)) * (3 * CC) ** -0.5).to(BF)
        self.x = (torch.randn(M, CC, generator=g(seed)) * 1.5 + 0.7 + 0.5 * torch.randn(Bn, 1, 1, generator=g(seed + 8)).expand(Bn, self.rps, 1).reshape(M, 1)).to(BF)
        self.bias = torch.randn(N, generator=g(seed + 2)) if bias else None
        self.ldo = N + 24 if pad else N
        self.ldr = N + 8 if pad else N
        self.res = (torch.randn(M, self.ldr, generator=g(seed + 4))).to(BF) if res else None
        self.gamma, self.beta = 1 + 0.2 * torch.randn(CC, generator=g(seed + 5)), 0.3 * torch.randn(CC, generator=g(seed + 6))
        d = "cuda"
        self.d = dict(x=self.x.to(d), w=P.pack_tconv(self.wt.float(), d), b=None if self.bias is None else self.bias.to(d),
                      res=None if self.res is None else self.res.to(d), y=torch.zeros(M, CC, dtype=BF, device=d), tab=torch.zeros(Bn * 2 * CC, device=d),
                      gamma=self.gamma.to(d), beta=self.beta.to(d), ws=torch.zeros(ops.gn_partial_floats(M, self.rps, CC), device=d))
        self.S = ops.Stream(record=False)
        self.S.groupnorm_stats(self.gnp(self.d["tab"], False), "stats")
        self.S.groupnorm_table(self.gnp(self.d["tab"], False), "table")

    def gnp(self, y, silu):
        t = self.d
        return ops.gn_params(t["x"], CC, CC, self.M, self.rps, t["ws"], t["gamma"], t["beta"], 1e-5, silu, y, CC)

    def out(self):
        return torch.full((self.M, self.ldo), SENT, dtype=BF, device="cuda")

    def params(self, src, out, tile, fold=False, silu=False):
        t = self.d
        kw = dict(gn_table=t["tab"], gn_rows_per_stat=self.rps, gn_silu=silu) if fold else {}
        return ops.gemm_params(self.M, self.N, ops.temporal_segs(src, CC, CC), t["w"], out, self.ldo, bias=t["b"], geom=ops.Geom(F=self.F, P=self.P),
                               residual=t["res"], ldr=self.ldr if t["res"] is not None else 0, tile=tile, **kw)

    def run(self, p, blocks=0):
        lib = self.S.lib
        assert lib.vmv_gemm_validate(C.byref(p)) == 0
        if blocks:
            rc = lib.vmv_gemm_trs_blocks(C.byref(p), blocks, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
        else:
            self.S.gemm(p, "gemm")
        torch.cuda.synchronize()

    def reference(self, fold, silu):
        xn = fold_ref(self.x, self.d["tab"].cpu(), self.rps, silu) if fold else self.x
        res = None if self.res is None else self.res[:, :self.N]
        return conv_ref64(xn, self.wt, self.bias, res, self.Bn, self.F, self.P, self.N)


# (Bn, F, P, N, fold, silu, bias, res, padded ldo / ldr, grid cap) — the smallest shapes at which each part of the kernel can go wrong
CASES = {
    "full-waves": (1, 24, 16, 320, True, True, True, False, False, 0),       # one block, all eight waves full
    "ragged-odd": (1, 24, 7, 320, True, True, True, True, True, 0),          # odd pixel count: a half-filled wave, waves of padding only
    "sample-seam": (2, 24, 9, 320, True, True, True, False, True, 0),        # a wave's two pixels in different samples: per-row table
    "f12": (1, 12, 21, 320, True, False, True, True, False, 0),              # shift by 4 rows, no SiLU
    "f16-n64": (2, 16, 11, 64, True, True, False, False, True, 0),           # shift by 3 rows, one column group, no bias
    "n96": (1, 24, 5, 96, True, True, True, True, True, 0),                  # N % 64 == 32: the last group has one pair
    "ranges": (1, 24, 40, 320, True, True, True, True, False, 4),            # 3 row tiles x 5 groups on 4 blocks: ranges cross row tiles
    "ranges-f12": (2, 12, 37, 320, True, True, True, False, True, 3),        # the same with two samples inside a block's range
    "plain": (2, 12, 9, 320, False, False, True, True, True, 0),             # the unfolded form (forced tile only)
    "plain-nobias": (1, 16, 6, 64, False, False, False, False, False, 0),
}


@pytest.mark.parametrize("key", list(CASES))
def test_trs_matches_fp64_and_the_two_launch_form(key):
    Bn, F_, Pp, N, fold, silu, bias, res, pad, blocks = CASES[key]
    c = Tc(Bn, F_, Pp, N, bias=bias, res=res, pad=pad)
    lib = c.S.lib
    # (a) the new kernel, folded (or plain) on the raw tensor
    out_a = c.out()
    pa = c.params(c.d["x"], out_a, L.TRS_TILE, fold=fold, silu=silu)
    assert lib.vmv_gemm_served_tile(C.byref(pa)) == L.TRS_TILE
    c.run(pa, blocks)
    # (b) the path it replaces: vmv_groupnorm_apply + the 256 x 320 tile (the policy's tile where that one does not serve the shape)
    src_b = c.d["x"]
    if fold:
        c.S.groupnorm_apply(c.gnp(c.d["y"], silu), "apply")
        src_b = c.d["y"]
    out_b = c.out()
    pb = c.params(src_b, out_b, L.TILE_X256x320)
    if lib.vmv_gemm_validate(C.byref(pb)) != 0 or lib.vmv_gemm_served_tile(C.byref(pb)) != L.TILE_X256x320:
        pb = c.params(src_b, out_b, L.TILE_AUTO)
    c.run(pb)
    ref = c.reference(fold, silu)
    ea, eb = rel_l2_64(out_a[:, :N], ref), rel_l2_64(out_b[:, :N], ref)
    print(f"trs[{key}] {L.elem_name()}: rel-L2 vs fp64  new kernel {ea:.3e}  old path {eb:.3e}  ratio {ea / eb:.3f}")
    assert torch.isfinite(out_a[:, :N].float()).all()
    assert ea <= 1.5 * eb, (key, ea, eb)
    # the pad columns of a padded output are untouched, bit for bit
    if pad:
        assert torch.equal(out_a[:, N:], torch.full_like(out_a[:, N:], SENT))
    # operand identity: the folded launch == vmv_groupnorm_apply followed by the unfolded launch on the same kernel, bit for bit
    if fold:
        out_c = c.out()
        pc = c.params(c.d["y"], out_c, L.TRS_TILE)
        c.run(pc, blocks)
        assert torch.equal(out_a, out_c)


@pytest.mark.parametrize("F_,Pp,Bn", [(24, 5, 1), (16, 7, 2), (12, 9, 1)])
def test_trs_impulses_are_exact(F_, Pp, Bn):
    """One nonzero activation, W a 0 / 1 selection matrix (tap t of input channel c0 -> the output channels n with n % 3 == t), no norm:
    an impulse at frame 0, F - 1 or inside appears at the right one / two / three frames of ITS pixel and nowhere else — not in the
    neighbouring pixels of the wave (the seam of the frame-major rows), not in the other sample, not in the zero fill of the shift."""
    N, c0 = 64, 37
    M = Bn * F_ * Pp
    wt = torch.zeros(N, CC, 3, 1, 1)
    for n in range(N):
        wt[n, c0, n % 3] = 1.0
    dev = "cuda"
    w = P.pack_tconv(wt, dev)
    S = ops.Stream(record=False)
    ppw = 48 // F_
    pixels = sorted({0, 1, ppw - 1, ppw, Pp - 1})                    # first / last pixel of a wave, the first of the next wave, the last
    for b in range(Bn):
        for px in pixels:
            for f in (0, F_ - 1, F_ // 2):
                x = torch.zeros(M, CC, dtype=BF)
                x[(b * F_ + f) * Pp + px, c0] = 1.0
                xd = x.to(dev)
                out = torch.full((M, N), SENT, dtype=BF, device=dev)
                p = ops.gemm_params(M, N, ops.temporal_segs(xd, CC, CC), w, out, N, geom=ops.Geom(F=F_, P=Pp), tile=L.TRS_TILE)
                assert S.lib.vmv_gemm_served_tile(C.byref(p)) == L.TRS_TILE
                S.gemm(p, "impulse")
                torch.cuda.synchronize()
                ref = conv_ref64(x, wt.to(BF), None, None, Bn, F_, Pp, N)
                assert torch.equal(out.double().cpu(), ref), (b, px, f, (out.double().cpu() - ref).nonzero()[:8].tolist())


def test_trs_policy_dispatch(monkeypatch):
    """tile = VMV_TILE_AUTO reaches the kernel for the folded form once VMV_TRS_MIN_ITEMS allows the shape, and gives the forced launch's bits"""
    c = Tc(2, 24, 9, 320)
    lib = c.S.lib
    out0 = c.out()
    p = c.params(c.d["x"], out0, L.TILE_AUTO, fold=True, silu=True)
    assert lib.vmv_gemm_trs_ok(C.byref(p)) == 0 and lib.vmv_gemm_served_tile(C.byref(p)) == L.TILE_TFR      # 10 items: under the threshold
    monkeypatch.setenv("VMV_TRS_MIN_ITEMS", "1")
    assert lib.vmv_gemm_trs_ok(C.byref(p)) == 1 and lib.vmv_gemm_served_tile(C.byref(p)) == L.TRS_TILE
    c.run(p)
    out1 = c.out()
    c.run(c.params(c.d["x"], out1, L.TRS_TILE, fold=True, silu=True))
    assert torch.equal(out0, out1)


def test_trs_other_element_type_in_child_process():
    """the same checks through the library of the other 16-bit type, for one shape (a process loads one library: tests/test_bf16_gpu.py)"""
    if os.environ.get("VMV_DTYPE_CHILD"):
        pytest.skip("already the child run")
    other = "bf16" if L.elem_name() == "fp16" else "fp16"
    env = dict(os.environ, VMV_DTYPE=other, VMV_DTYPE_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_trs_gpu.py", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "sample-seam or ranges-f12 or impulses"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("trs[")))
