"""TEST INFRASTRUCTURE: the phased nearest-x2 + 3x3 convolution (include/vmv.h: VmvGemmParams.phased) written out in plain torch from the
header's contract — gather the 2 x 2 window of every source pixel per output phase, four matmuls, scatter to the output rows — and an
executor of a phased argument block on host memory (tests/plan_interp.py, which stays as it is, executes the nine-tap form only)."""
import torch

from videomv_amd import _lib as L
from tests import plan_interp as I

TAPS = [(-1, -1), (-1, 0), (0, -1), (0, 0)]


def up4_rows(a, n, IH, IW, W4, bias=None):
    """a: source rows [n * IH * IW, C]; W4: [4, N, 4 * C] (phase, output channel, (tap, channel)); -> output rows [n * 2IH * 2IW, N] in a's dtype."""
    Mp, N = n * IH * IW, W4.shape[1]
    assert a.shape[0] == Mp
    OH, OW = 2 * IH, 2 * IW
    r = torch.arange(Mp)
    img, rem = r // (IH * IW), r % (IH * IW)
    i, j = rem // IW, rem % IW
    out = torch.zeros(n * OH * OW, N, dtype=a.dtype)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        cols = []
        for d0, d1 in TAPS:
            y, x = i + py + d0, j + px + d1
            valid = (y >= 0) & (y < IH) & (x >= 0) & (x < IW)
            t = a[img * IH * IW + y.clamp(0, IH - 1) * IW + x.clamp(0, IW - 1)].clone()
            t[~valid] = 0
            cols.append(t)
        acc = torch.cat(cols, dim=1) @ W4[ph].t()
        if bias is not None:
            acc = acc + bias
        out[(img * OH + 2 * i + py) * OW + 2 * j + px] = acc
    return out


def gemm_phased(p: L.GemmParams):
    """Execute a phased GEMM argument block on host memory (fp32 accumulation, 16-bit output, as plan_interp.gemm does for the other modes)."""
    assert p.phased == 1 and p.nseg == 4 and p.ups == 1 and p.stride == 1 and not p.out_fp32
    assert [(p.seg[s].d0, p.seg[s].d1) for s in range(4)] == TAPS and all(p.seg[s].src == p.seg[0].src for s in range(4))
    assert not (p.residual or p.rowvec or p.rowstat or p.colsum or p.gn_table or p.wgroup_rows or p.epilogue)
    k, N = p.seg[0].k, p.N
    Mp = p.M // 4
    n = Mp // (p.IH * p.IW)
    assert p.ktot == 4 * k and p.M == 4 * n * p.IH * p.IW and p.OH == 2 * p.IH and p.OW == 2 * p.IW
    a = I._rows(p.seg[0].src, Mp, p.seg[0].ld)[:, :k].float()
    W4 = I._rows(p.W, 4 * N, p.ktot).float().view(4, N, p.ktot)
    bias = I._view(p.bias, N, "f32") if p.bias else None
    acc = up4_rows(a, n, p.IH, p.IW, W4, bias)
    if p.act == L.ACT_SILU:
        acc = torch.nn.functional.silu(acc)
    elif p.act == L.ACT_GELU:
        acc = torch.nn.functional.gelu(acc)
    I._rows(p.out, p.M, p.ldo)[:, :N] = acc.to(L.elem())


def install(monkeypatch):
    """plan_interp.install + phased blocks executed by gemm_phased."""
    I.install(monkeypatch)
    plain = I.gemm
    monkeypatch.setattr(I, "gemm", lambda p: gemm_phased(p) if p.phased else plain(p))
