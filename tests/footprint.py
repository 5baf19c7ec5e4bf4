"""TEST INFRASTRUCTURE: the store footprint and the read footprint of a launch, made visible.

Production never runs a kernel on a dense [M][N] buffer: GEMMs write head slices and padded rows of wider activations and read slices
of wider rows.  A store that strays past column N of a row, or past row M of the last tile, then lands in live data, and a read past
column k reads a neighbour.  Here every operand of a launch lives in an ARENA, one larger allocation:

    output   G_before guard rows | M payload rows | G_after guard rows, every row `ld` elements wide, the kernel's pointer `col_off`
             elements into payload row 0; everything outside the payload columns [col_off, col_off + width) of the payload rows holds
             a fixed finite bit pattern (PAT16 / PAT32) that is compared BIT FOR BIT after the launch — no tolerance;
    input    the same shape, everything outside the columns and rows the contract says are read is NaN: a kernel that reads a
             neighbour's columns, or multiplies a wrongly addressed row by zero instead of not reading it, produces a non-finite payload.

G_after >= 512 (the largest BM of any kernel), so a whole overshooting tail tile still lands inside the allocation and is reported with
its coordinates instead of faulting.  The reference of every case is tests/plan_interp.py (tests/up4_ref.py for the phased form) run on
a host copy of the same arenas; the case builders below are shared by tests/test_footprint_gpu.py (the kernels) and
tests/test_footprint_cpu.py (the arena arithmetic and the reference, no GPU).  Plain Python: no fixtures, no pytest settings.
"""
import ctypes as C

import torch

from videomv_amd import _lib as L
from videomv_amd import ops, packing as P
from tests import plan_interp as I
from tests import up4_ref

# 0x7B5A: fp16 60224, bf16 1.13e36 — finite in both, far outside what a case produces (|outputs| < 100; fp16 saturation stores 0x7BFF);
# the fp32 pattern repeats it, so a 16-bit store into an fp32 guard is seen too
PAT16 = 0x7B5A
PAT32 = 0x7B5A7B5A
G_BEFORE, G_AFTER = 8, 512
G_SRC = 64          # guard rows before a gathered source: a tap that is addressed before it is masked reaches IW + 1 (P) rows back

KINDS = {"elem": (lambda: L.elem(), torch.int16, PAT16), "f32": (lambda: torch.float32, torch.int32, PAT32)}


def g(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=g(seed)) * scale


class Arena:
    """One operand: `rows` x `width` payload inside (g_before + rows + g_after) rows of `ld` elements, the payload `col_off` columns in.
    poison = "guard": the rest holds the bit pattern (outputs, workspaces);  "nan": the rest is NaN (inputs)."""

    def __init__(self, rows, width, kind="elem", ld=None, col_off=0, g_before=G_BEFORE, g_after=G_AFTER, poison="guard", data=None, tile=(1, 1)):
        ld = width if ld is None else ld
        assert col_off >= 0 and col_off + width <= ld and g_before >= 0 and g_after >= (1 if col_off else 0)
        self.rows, self.width, self.kind, self.ld, self.col_off, self.gb, self.ga, self.poison, self.tile = rows, width, kind, ld, col_off, g_before, g_after, poison, tile
        dt, it, pat = KINDS[kind]
        self.dtype, self.itype = dt(), it
        total = (g_before + rows + g_after) * ld
        if poison == "guard":
            buf = torch.full((total,), pat, dtype=it).view(self.dtype)
        else:
            buf = torch.full((total,), float("nan"), dtype=self.dtype)
        self.buf = buf
        pay = self.payload(buf)
        if data is None:
            pay.zero_()
        else:
            assert tuple(data.shape) == (rows, width), (data.shape, rows, width)
            pay.copy_(data.to(self.dtype))

    @property
    def offset(self):           # elements from the allocation's start to the kernel's pointer
        return self.gb * self.ld + self.col_off

    def ptr(self, buf):
        return buf.data_ptr() + self.offset * buf.element_size()

    def payload(self, buf):
        return buf.view(-1, self.ld)[self.gb:self.gb + self.rows, self.col_off:self.col_off + self.width]

    def holds(self, first_elem, n_elem):
        """is [first, first + n) elements, counted from the kernel's pointer, inside the allocation?"""
        return 0 <= self.offset + first_elem and self.offset + first_elem + n_elem <= self.buf.numel()

    def stray(self, buf, limit=8):
        """coordinates of the first non-payload elements that no longer hold the guard pattern: [(arena row, arena column, tile row, tile column)]"""
        assert self.poison == "guard"
        bits = buf.detach().cpu().contiguous().view(self.itype).view(-1, self.ld)
        bad = bits != KINDS[self.kind][2]
        bad[self.gb:self.gb + self.rows, self.col_off:self.col_off + self.width] = False
        idx = bad.nonzero()[:limit].tolist()
        bm, bn = self.tile
        return [(r, c, (r - self.gb) // bm, (c - self.col_off) // bn) for r, c in idx]


def stray_report(name, arena, buf):
    bad = arena.stray(buf)
    if not bad:
        return ""
    return (f"{name}: stores outside the payload (payload rows [{arena.gb}, {arena.gb + arena.rows}) x columns [{arena.col_off}, "
            f"{arena.col_off + arena.width}) of an arena {arena.ld} wide; tile {arena.tile[0]} x {arena.tile[1]}): "
            + ", ".join(f"arena (row {r}, col {c}) = tile (row {tr}, col {tc})" for r, c, tr, tc in bad))


class Bound:
    """A case's operands on one device: b["name"] = the kernel's pointer of an arena (int) or a dense tensor; b.buf / b.payload by name."""

    def __init__(self, case, dev):
        self.case = case
        self.bufs = {k: a.buf.clone().to(dev) for k, a in case.arenas.items()}
        self.dense = {k: v.clone().to(dev).contiguous() for k, v in case.dense.items()}

    def __getitem__(self, k):
        if k in self.bufs:
            return self.case.arenas[k].ptr(self.bufs[k])
        return self.dense[k]

    def buf(self, k):
        return self.bufs[k]

    def payload(self, k):
        return self.case.arenas[k].payload(self.bufs[k])


class FCase:
    """One launch: arenas + dense operands, `build(b)` -> the argument block(s) from a Bound, `ref(args)` runs the interpreter on
    them (host), `gpu(lib, args, stream)` the kernel.  outs = {arena name: check() keywords, or "exact"}."""

    def __init__(self, name, arenas, dense, build, ref, gpu, outs, tile=0):
        self.name, self.arenas, self.dense, self.build, self.ref, self.gpu, self.outs, self.tile = name, arenas, dense, build, ref, gpu, outs, tile

    def on(self, dev):
        return Bound(self, dev)

    def run_ref(self):
        b = self.on("cpu")
        self.ref(self.build(b))
        return b

    def run_gpu(self):
        b = self.on("cuda")
        lib = L.load()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.gpu(lib, self.build(b), st)
        torch.cuda.synchronize()
        assert rc == 0, f"{self.name}: launch returned {rc}"
        return b

    def inputs_report(self, b):
        """"" when every input arena (NaN around the columns and rows that are read) of the bound case still holds, bit for bit, what it
        held before the launch: a kernel must not store into a source, residual or row-vector arena, inside its payload or outside"""
        bad = [k for k, a in self.arenas.items() if a.poison == "nan" and not torch.equal(b.buf(k).cpu().view(a.itype), a.buf.view(a.itype))]
        return ", ".join(f"{self.name}.{k}: the launch wrote into an input arena" for k in bad)

    def guards_report(self, b):
        """"" when every guarded arena of the bound case is intact, else the first stray coordinates of each"""
        return "\n".join(r for r in (stray_report(f"{self.name}.{k}", a, b.buf(k)) for k, a in self.arenas.items() if a.poison == "guard") if r)


# ------------------------------------------------------------------------------------------------- GEMM family
# every live tile id: name -> (BM, BN) of its kernel
TILES = {
    "128x128": (128, 128), "128x160": (128, 160), "128x64": (128, 64), "64x64": (64, 64),
    "256x128": (256, 128), "256x160": (256, 160), "G128x128": (128, 128), "G128x160": (128, 160),
    "P256x128": (256, 128), "P256x160": (192, 160), "PP256x128": (256, 128), "PP256x160": (256, 160),
    "Q128x128": (128, 128), "Q96x160": (96, 160),
    "X256x320": (256, 320), "X256x256": (256, 256), "X256x128": (256, 128), "X512x128": (512, 128),
    "RS": (512, 64), "RS512": (512, 64), "RS256": (256, 64), "HALO": (64, 8), "TFR": (192, 320), "TQA": (48, 192),
}
RETIRED = ("S256x128", "S192x160", "S256x160", "A128x160", "A128x128", "W256x256", "Y256x128")
GENERIC = [t for t in TILES if t not in ("RS", "RS512", "RS256", "HALO", "TFR", "TQA")]


def tile_id(name):
    return getattr(L, "TILE_" + name)


# layouts of the generic matrix (the issue's letters): what differs from the dense launch
LAYOUTS = ("a", "b", "c", "d", "d2", "e", "f", "g_s1", "g_s2", "g_ups", "g_t", "h", "i", "j", "k_rowstat", "k_inline")
# layouts whose padded launch takes the dense launch's store path (ldo % 8 == 0, N_out % 8 == 0, 16-bit) and does not split K:
# the padded payload must be BIT-identical to the dense one
BITWISE = ("a", "d", "d2", "e", "f", "g_s1", "g_s2", "g_ups", "g_t", "i", "j", "k_rowstat", "k_inline")


def _imgs(bm):
    return (bm + 1 + 129) // 130


def gemm_case(tname, layout, dense=False):
    """The case of the generic matrix for tile `tname` and `layout`; dense=True: the same operands and tile in dense buffers (the
    bit-identity twin).  Shapes: one full row tile + a ragged tail (M = BM + 1 for plain rows; whole images / frames otherwise: the
    smallest count past BM), one full column tile + an 8-column tail, >= 2 K chunks of every kernel."""
    bm, bn = TILES[tname]
    tile = tile_id(tname)
    geglu = layout == "f"
    fp32 = layout == "c"
    n_img = _imgs(bm)
    geom, mode = None, "linear"
    K = 256 if layout == "h" else 128
    if layout in ("g_s1", "g_s2", "j"):
        mode, OH, OW = "spatial", 10, 13
        IH, IW, stride, ups = (19, 25, 2, 0) if layout == "g_s2" else (10, 13, 1, 0)
        Mrows = n_img * OH * OW
        if layout == "j":                     # phased: the source image is IH x IW, the output 2 IH x 2 IW; M = 4 Mp
            OH, OW, ups = 20, 26, 1
            Mrows = 4 * n_img * IH * IW
        geom = ops.Geom(OH=OH, OW=OW, IH=IH, IW=IW, stride=stride, ups=ups)
        src_rows, K = n_img * IH * IW, 64
    elif layout == "g_ups":
        mode, OH, OW, IH, IW = "spatial", 10, 14, 5, 7
        n_img = (bm + 1 + 139) // 140
        Mrows, src_rows, K = n_img * 140, n_img * 35, 64
        geom = ops.Geom(OH=OH, OW=OW, IH=IH, IW=IW, stride=1, ups=1)
    elif layout == "g_t":
        mode, F_, Pp = "temporal", 5, 26
        Mrows = src_rows = n_img * F_ * Pp
        geom, K = ops.Geom(F=F_, P=Pp), 64
    elif layout == "i":
        Mrows = src_rows = 512             # G = 2 groups of R = 256 rows
    else:
        Mrows = src_rows = bm + 1
    M = Mrows
    N = bn + 32 if geglu else bn + 8
    No = N // 2 if geglu else N
    # ---- sources
    pad_src = (not dense) and layout in ("d", "d2", "g_s1", "g_s2", "g_ups", "g_t", "j", "k_inline", "k_rowstat")
    ln = layout in ("k_rowstat", "k_inline")
    arenas, dn = {}, {}
    if layout == "d2":                    # channel concat: two sources of different row strides
        ks = [(K // 2, 8, 8), (K // 2, 24, 16)]
    else:
        ks = [(K, 8, 8)]
    srcs = []
    for i, (k, pad, off) in enumerate(ks):
        x = rnd((src_rows, k), 11 + i)
        if ln:
            x = 1.5 * x + 4.0 * rnd((src_rows, 1), 19)
        arenas[f"x{i}"] = Arena(src_rows, k, "elem", ld=k + pad if pad_src else k, col_off=off if pad_src else 0, g_before=G_SRC, poison="nan", data=x)
        srcs.append((f"x{i}", k + pad if pad_src else k, k))
    nseg_k = {"linear": 1, "spatial": 9, "temporal": 3}[mode] if layout != "j" else 4
    ktot = nseg_k * sum(k for k, _, _ in ks)
    groups = 2 if layout == "i" else 1
    phases = 4 if layout == "j" else 1
    # ---- weights: rows past N are legal reads (vmv.h) and hold ordinary finite values whose products must never be stored
    w = rnd((groups * phases * N + 512, ktot), 2, ktot ** -0.5)
    bias = rnd((N + 512,), 3)
    colsum = None
    if ln:
        gamma, beta = 1 + 0.2 * rnd((K,), 4), 0.2 * rnd((K,), 5)
        wf, bf, cs = P.fold_layernorm(w[:N], bias[:N], gamma, beta)
        w, bias = torch.cat([wf.float(), w[N:]]), torch.cat([bf.float(), bias[N:]])
        colsum = torch.cat([cs.float(), torch.zeros(512)])
    if layout == "j":
        wt = rnd((N, K, 3, 3), 2, (9 * K) ** -0.5)
        w = torch.cat([P.pack_conv3x3_up4(wt, "cpu").float().view(4 * N, 4 * K), rnd((512, 4 * K), 6, 0.05)])
    dn["w"], dn["bias"] = w.to(L.elem()), bias
    if colsum is not None:
        dn["colsum"] = colsum
    if layout == "k_rowstat":
        xf = arenas["x0"].payload(arenas["x0"].buf).float()
        dn["rowstat"] = torch.cat([torch.stack([xf.mean(dim=1), torch.rsqrt(xf.var(dim=1, unbiased=False) + 1e-5)], dim=1), torch.zeros(512, 2)]).contiguous()
    # ---- output
    if dense:
        ldo, ooff = No, 0
    elif layout in ("b", "c"):
        ldo, ooff = No + 4, 0
    else:
        ldo, ooff = No + 8, 8
    arenas["out"] = Arena(M, No, "f32" if fp32 else "elem", ld=ldo, col_off=ooff, tile=(bm, bn // 2 if geglu else bn))
    res = layout in ("e", "h")
    if res:
        arenas["res"] = Arena(M, No, "elem", ld=No if dense else No + 8, col_off=0 if dense else 8, poison="nan", data=rnd((M, No), 5))
    # a row vector per 64 rows (five row groups under a 256-row tile); per 128 rows for the 512-row tile, which stages as many
    rv_div = 128 if bm == 512 else 64
    if layout == "e":
        ngrp = (M + rv_div - 1) // rv_div
        arenas["rv"] = Arena(ngrp, No, "f32", ld=No if dense else No + 8, col_off=0 if dense else 4, poison="nan", data=rnd((ngrp, No), 7))
    ksplit = 2 if layout == "h" else 0
    if ksplit:
        arenas["ws"] = Arena(ksplit * M, N, "f32", tile=(bm, bn))

    def build(b):
        sl = [(b[n_], ld, k) for n_, ld, k in srcs]
        if layout == "j":
            segs = ops.up4_segs(sl[0][0], sl[0][1], sl[0][2])
        elif mode == "spatial":
            segs = ops.conv3x3_segs(sl)
        elif mode == "temporal":
            segs = ops.temporal_segs(*sl[0])
        else:
            segs = ops.linear_segs(sl)
        kw = {}
        if res:
            kw.update(residual=b["res"], ldr=arenas["res"].ld)
        if layout == "e":
            kw.update(rowvec=b["rv"], rowvec_div=rv_div, rowvec_ld=arenas["rv"].ld, act=L.ACT_SILU)
        if ksplit:
            kw.update(ksplit=ksplit, workspace=b["ws"])
        if groups > 1:
            kw.update(wgroup_rows=256, wgroup_stride=N * ktot)
        if layout == "k_rowstat":
            kw.update(rowstat=b["rowstat"], colsum=b["colsum"])
        if layout == "k_inline":
            kw.update(colsum=b["colsum"], ln_eps=1e-5)
        return ops.gemm_params(M, N, segs, b["w"], b["out"], ldo, bias=b["bias"], out_fp32=fp32, geom=geom, tile=tile,
                               epilogue=L.EPI_GEGLU if geglu else L.EPI_NONE, phased=layout == "j", **kw)

    tol = dict(tol_l2=1e-3, tol_max=2e-3) if fp32 else dict(tol_l2=6e-3, tol_max=2e-2) if ln else {}
    return FCase(f"gemm[{tname}-{layout}{'-dense' if dense else ''}]", arenas, dn, build,
                 lambda p: up4_ref.gemm_phased(p) if p.phased else I.gemm(p), lambda lib, p, st: lib.vmv_gemm(C.byref(p), st), {"out": tol}, tile=tile)


# row-stationary kernel: K in {320, 640, 512}, N % 64 == 0; 64 rows per wave (RS512, K = 320 only) and 32 (RS256); N = 128 splits the
# columns over two blocks per row tile, N = 64 / 192 cannot be split
RS_CASES = {
    "RS512-a": ("RS512", 513, 128, 320, "a"), "RS512-nosplit": ("RS512", 513, 64, 320, "a"), "RS256-a": ("RS256", 257, 128, 640, "a"),
    "RS256-k512": ("RS256", 257, 192, 512, "a"), "RS-a": ("RS", 513, 128, 320, "a"), "RS256-k320": ("RS256", 257, 64, 320, "a"),
    "RS512-d": ("RS512", 513, 128, 320, "d"), "RS256-d": ("RS256", 257, 128, 640, "d"),
    "RS512-res": ("RS512", 513, 128, 320, "res"), "RS256-res": ("RS256", 257, 128, 640, "res"),
    "RS512-f": ("RS512", 513, 256, 320, "f"), "RS256-f": ("RS256", 257, 256, 640, "f"),
    "RS512-k_inline": ("RS512", 513, 128, 320, "k_inline"), "RS256-k_inline": ("RS256", 257, 128, 640, "k_inline"),
    "RS512-l": ("RS512", 1056, 128, 320, "l"), "RS256-l": ("RS256", 1056, 128, 640, "l"),
}


def rs_case(key, dense=False):
    tname, M, N, K, layout = RS_CASES[key]
    bm = TILES[tname][0]
    geglu, ln = layout == "f", layout == "k_inline"
    No = N // 2 if geglu else N
    pad = not dense
    x = rnd((M, K), 11)
    if ln:
        x = 1.5 * x + 4.0 * rnd((M, 1), 19)
    arenas = {"x0": Arena(M, K, "elem", ld=K + 8 if pad else K, col_off=8 if pad else 0, poison="nan", data=x)}
    w, bias = rnd((N + 512, K), 2, K ** -0.5), rnd((N + 512,), 3)
    dn = {}
    if ln:
        wf, bf, cs = P.fold_layernorm(w[:N], bias[:N], 1 + 0.2 * rnd((K,), 4), 0.2 * rnd((K,), 5))
        w, bias = torch.cat([wf.float(), w[N:]]), torch.cat([bf.float(), bias[N:]])
        dn["colsum"] = torch.cat([cs.float(), torch.zeros(512)])
    rps = 528                                # stat groups of whole 16-row tiles that straddle the 256- / 512-row blocks
    if layout == "l":
        nstat = M // rps
        dn["tab"] = torch.stack([1 + 0.2 * rnd((nstat + 2, K), 8), 0.1 * rnd((nstat + 2, K), 9)], dim=1).contiguous()      # (two spare groups: a tile's rows past M)
    dn["w"], dn["bias"] = w.to(L.elem()), bias
    ldo, ooff = (No + 8, 8) if pad else (No, 0)
    arenas["out"] = Arena(M, No, "elem", ld=ldo, col_off=ooff, tile=(bm, 64))
    if layout == "res":
        arenas["res"] = Arena(M, No, "elem", ld=No + 8 if pad else No, col_off=8 if pad else 0, poison="nan", data=rnd((M, No), 5))

    def build(b):
        kw = {}
        if layout == "res":
            kw.update(residual=b["res"], ldr=arenas["res"].ld, res_scale=0.5)
        if ln:
            kw.update(colsum=b["colsum"], ln_eps=1e-5)
        if layout == "l":
            kw.update(gn_table=b["tab"], gn_rows_per_stat=rps)
        return ops.gemm_params(M, N, ops.linear_segs([(b["x0"], arenas["x0"].ld, K)]), b["w"], b["out"], ldo, bias=b["bias"], tile=tile_id(tname),
                               epilogue=L.EPI_GEGLU if geglu else L.EPI_NONE, **kw)

    tol = dict(tol_l2=6e-3, tol_max=2e-2) if ln else {}
    return FCase(f"gemm[{key}{'-dense' if dense else ''}]", arenas, dn, build, I.gemm, lambda lib, p, st: lib.vmv_gemm(C.byref(p), st), {"out": tol},
                 tile=tile_id(tname))


# frame-resident temporal convolution: 12 <= F <= 24, N % 320 == 0, C % 64 == 0; 192 / F pixels per block, P = 17 leaves the last block
# with one pixel (F = 12) / P = 11 with three (F = 24)
TFR_CASES = {"TFR-a": (1, 12, 17, 64, 320, "a"), "TFR-a2": (2, 24, 11, 128, 640, "a"), "TFR-e": (1, 12, 17, 64, 320, "res"), "TFR-l": (2, 12, 17, 64, 320, "l"),
             "TFR-l-silu": (1, 24, 11, 64, 320, "l_silu")}


def tfr_case(key, dense=False):
    Bn, F_, Pp, Cc, N, layout = TFR_CASES[key]
    M = Bn * F_ * Pp
    pad = not dense
    gn = layout in ("l", "l_silu")
    arenas = {"x0": Arena(M, Cc, "elem", ld=Cc + 8 if pad else Cc, col_off=8 if pad else 0, g_before=G_SRC, poison="nan", data=rnd((M, Cc), 11) + (0.3 if gn else 0.0))}
    dn = {"w": rnd((N + 512, 3 * Cc), 2, (3 * Cc) ** -0.5).to(L.elem()), "bias": rnd((N + 512,), 3)}
    if gn:
        dn["tab"] = torch.stack([1 + 0.2 * rnd((Bn + 2, Cc), 8), 0.1 * rnd((Bn + 2, Cc), 9)], dim=1).contiguous()
    ldo, ooff = (N + 8, 8) if pad else (N, 0)
    arenas["out"] = Arena(M, N, "elem", ld=ldo, col_off=ooff, tile=(192 // F_ * F_, 320))
    if layout == "res":
        arenas["res"] = Arena(M, N, "elem", ld=N + 8 if pad else N, col_off=8 if pad else 0, poison="nan", data=rnd((M, N), 5))

    def build(b):
        kw = {}
        if layout == "res":
            kw.update(residual=b["res"], ldr=arenas["res"].ld)
        if gn:
            kw.update(gn_table=b["tab"], gn_rows_per_stat=F_ * Pp, gn_silu=layout == "l_silu")
        return ops.gemm_params(M, N, ops.temporal_segs(b["x0"], arenas["x0"].ld, Cc), b["w"], b["out"], ldo, bias=b["bias"], geom=ops.Geom(F=F_, P=Pp),
                               tile=L.TILE_TFR, **kw)

    tol = dict(tol_l2=6e-3, tol_max=2.5e-2) if gn else {}
    return FCase(f"gemm[{key}{'-dense' if dense else ''}]", arenas, dn, build, I.gemm, lambda lib, p, st: lib.vmv_gemm(C.byref(p), st), {"out": tol}, tile=L.TILE_TFR)


# fused q | k | v + temporal attention: K = 320, 48 % F == 0; pixel counts that leave the last wave ragged
TQA_CASES = {"TQA-ln": (1, 24, 5, 2, True), "TQA-plain": (2, 12, 7, 1, False)}


def tqa_case(key, dense=False):
    nb, F_, Pp, heads, ln = TQA_CASES[key]
    K, inner = 320, 64 * heads
    M = nb * F_ * Pp
    pad = not dense
    x = 1.2 * rnd((M, K), 1) + 0.7 * rnd((M, 1), 9)
    w = rnd((3 * inner, K), 2, 1.6 * K ** -0.5)
    dn = {}
    if ln:
        wf, bf, cs = P.fold_layernorm(w, None, 1 + 0.2 * rnd((K,), 4), 0.2 * rnd((K,), 5))
        dn["bias"] = torch.cat([P.qkv_head_major(bf).float(), torch.zeros(512)])
        dn["colsum"] = torch.cat([P.qkv_head_major(cs).float(), torch.zeros(512)])
    else:
        wf = w
    dn["w"] = torch.cat([P.qkv_head_major(wf.float()), rnd((512, K), 6, 0.05)]).to(L.elem())
    arenas = {"x0": Arena(M, K, "elem", ld=K + 8 if pad else K, col_off=8 if pad else 0, poison="nan", data=x)}
    ldo, ooff = (inner + 16, 8) if pad else (inner, 0)
    arenas["out"] = Arena(M, inner, "elem", ld=ldo, col_off=ooff, tile=(48, 64))

    def build(b):
        kw = dict(bias=b["bias"], colsum=b["colsum"], ln_eps=1e-5) if ln else {}
        return ops.gemm_params(M, 3 * inner, ops.linear_segs([(b["x0"], arenas["x0"].ld, K)]), b["w"], b["out"], ldo, epilogue=L.EPI_TATTN, epi_scale=0.125,
                               geom=ops.Geom(F=F_, P=Pp), tile=L.TILE_TQA, **kw)

    return FCase(f"gemm[{key}{'-dense' if dense else ''}]", arenas, dn, build, I.gemm, lambda lib, p, st: lib.vmv_gemm(C.byref(p), st),
                 {"out": dict(tol_l2=8e-3, tol_max=3e-2)}, tile=L.TILE_TQA)


# halo-resident 3 x 3 convolution, N <= 8: images that are no multiple of the 4 x 16 pixel tile, fp32 and 16-bit outputs
HALO_CASES = {"HALO-f32": (2, 9, 17, 64, 4, True, 8, 4), "HALO-16": (1, 5, 19, 160, 8, False, 16, 8), "HALO-f32-n8": (1, 6, 33, 32, 8, True, 12, 4)}


def halo_case(key, dense=False):
    n, H, W, Cin, N, fp32, ldo, ooff = HALO_CASES[key]
    M = n * H * W
    pad = not dense
    if dense:
        ldo, ooff = N, 0
    arenas = {"x0": Arena(M, Cin, "elem", ld=Cin + 8 if pad else Cin, col_off=8 if pad else 0, g_before=G_SRC, poison="nan", data=rnd((M, Cin), 11))}
    dn = {"w": rnd((N + 512, 9 * Cin), 2, (9 * Cin) ** -0.5).to(L.elem()), "bias": rnd((N + 512,), 3)}
    arenas["out"] = Arena(M, N, "f32" if fp32 else "elem", ld=ldo, col_off=ooff, tile=(64, 8))

    def build(b):
        return ops.gemm_params(M, N, ops.conv3x3_segs([(b["x0"], arenas["x0"].ld, Cin)]), b["w"], b["out"], ldo, bias=b["bias"], out_fp32=fp32,
                               geom=ops.Geom(OH=H, OW=W, IH=H, IW=W), tile=L.TILE_HALO)

    tol = dict(tol_l2=1e-3, tol_max=2e-3) if fp32 else {}
    return FCase(f"gemm[{key}{'-dense' if dense else ''}]", arenas, dn, build, I.gemm, lambda lib, p, st: lib.vmv_gemm(C.byref(p), st), {"out": tol}, tile=L.TILE_HALO)


SPECIAL = {}
for _tab, _fn in ((RS_CASES, rs_case), (TFR_CASES, tfr_case), (TQA_CASES, tqa_case), (HALO_CASES, halo_case)):
    for _k in _tab:
        SPECIAL[_k] = _fn


def ff_case(M=257 + 16, ln=True, res=True, dense=False):
    """vmv_ff_fused, C = 320: 128-row blocks of 16 waves; M = 273 leaves the last block with 17 rows: one full 16-row wave pair tile and a
    ragged one"""
    Cc = 320
    pad = not dense
    x = 1.5 * rnd((M, Cc), 1) + (3.0 * rnd((M, 1), 9) if ln else 0.0)
    w1, b1 = rnd((8 * Cc, Cc), 2, Cc ** -0.5), rnd((8 * Cc,), 3)
    w2, b2 = rnd((Cc, 4 * Cc), 4, (4 * Cc) ** -0.5), rnd((Cc,), 5)
    if ln:
        w1f, b1f, _ = P.fold_layernorm(w1, b1, 1 + 0.2 * rnd((Cc,), 6), 0.2 * rnd((Cc,), 7))
    else:
        w1f, b1f = w1, b1
    dn = {"w1": P.geglu_interleave(w1f.float()).to(L.elem()), "b1": P.geglu_interleave(b1f.float()).contiguous(), "w2": P.ff_down_permute(w2).to(L.elem()), "b2": b2}
    ld, off = (Cc + 8, 8) if pad else (Cc, 0)
    arenas = {"x": Arena(M, Cc, "elem", ld=ld, col_off=off, poison="nan", data=x), "out": Arena(M, Cc, "elem", ld=ld, col_off=off, tile=(128, 320))}
    if res:
        arenas["res"] = Arena(M, Cc, "elem", ld=ld, col_off=off, poison="nan", data=rnd((M, Cc), 8))

    def build(b):
        return ops.ff_params(M, Cc, b["x"], ld, b["w1"], b["b1"], b["w2"], b["b2"], b["out"], ld, residual=b["res"] if res else None, ldr=ld if res else 0,
                             ln_eps=1e-5 if ln else 0.0)

    return FCase(f"ff[M={M},ln={ln},res={res}{'-dense' if dense else ''}]", arenas, dn, build, I.ff_fused, lambda lib, p, st: lib.vmv_ff_fused(C.byref(p), st),
                 {"out": dict(tol_l2=6e-3, tol_max=2e-2)})


# ------------------------------------------------------------------------------------------------- row kernels
SOFTMAX_SCALE = 512 ** -0.5          # the VAE attention's (AttnBlock, 512 channels)


def softmax_case(rows, n, kind="normal", dense=False):
    """vmv_softmax_rows on fp32 scores; kind: "normal" (the spread of q.k at 512 channels), "huge" (|s| ~ 1e4), "dominant" (one entry per
    row 40 / scale above the rest: probabilities (1, ~0, ...))"""
    s = rnd((rows, n), 21, 30.0)
    if kind == "huge":
        s = rnd((rows, n), 22, 1.0e4)
    elif kind == "dominant":
        s[torch.arange(rows), (torch.arange(rows) * 7 + 3) % n] += 40.0 / SOFTMAX_SCALE
    ld, off = (n, 0) if dense else (n + 4, 4)
    arenas = {"s": Arena(rows, n, "f32", ld=ld, col_off=off, poison="nan", data=s), "p": Arena(rows, n, "elem", ld=ld, col_off=off, tile=(4, n))}

    def build(b):
        return ops.softmax_params(b["s"], ld, b["p"], ld, rows, n, SOFTMAX_SCALE)

    def ref(p):          # fp64 softmax(scale * s) of the fp32 scores
        sc = I._rows(p.s, p.rows, p.lds, "f32")[:, : p.n].double()
        I._rows(p.p, p.rows, p.ldp)[:, : p.n] = torch.softmax(sc * float(p.scale), dim=-1).to(L.elem())

    return FCase(f"softmax[{rows}x{n}-{kind}]", arenas, {}, build, ref, lambda lib, p, st: lib.vmv_softmax_rows(C.byref(p), st), {"p": {}})


def layernorm_case(rows, Cc, stats=False, dense=False):
    """vmv_layernorm: the y form and the stats_out form ((mean, rstd) table, y = NULL)"""
    ld, off = (Cc, 0) if dense else (Cc + 8, 8)
    arenas = {"x": Arena(rows, Cc, "elem", ld=ld, col_off=off, poison="nan", data=2.0 * rnd((rows, Cc), 1) + 0.3)}
    dn = {"gamma": 1 + 0.1 * rnd((Cc,), 3), "beta": 0.1 * rnd((Cc,), 4)}
    if stats:
        arenas["st"] = Arena(rows, 2, "f32", tile=(4, 2))
    else:
        arenas["y"] = Arena(rows, Cc, "elem", ld=ld, col_off=off, tile=(4, Cc))

    def build(b):
        if stats:
            return ops.ln_params(b["x"], ld, None, 0, None, None, rows, Cc, 1e-5, stats_out=b["st"])
        return ops.ln_params(b["x"], ld, b["y"], ld, b["gamma"], b["beta"], rows, Cc)

    return FCase(f"layernorm[{rows}x{Cc}{'-stats' if stats else ''}]", arenas, dn, build, I.layernorm, lambda lib, p, st: lib.vmv_layernorm(C.byref(p), st),
                 {"st": "stats"} if stats else {"y": dict(tol_l2=5e-3, tol_max=1.5e-2)})


def groupnorm_case(form, rows=3 * 50, rps=50, C0=64, C1=64, silu=True, chunk_rows=16, dense=False):
    """vmv_groupnorm_stats + _apply ("apply"), _fused ("fused"), _stats + _table ("table") with two sources; rows_per_stat = 50 is no
    multiple of chunk_rows = 16 (a ragged last chunk); the partial workspace [nstat][nchunk][32][2] is guarded"""
    Cc = C0 + C1
    pad = 0 if dense else 8
    nstat, nchunk = rows // rps, (rps + chunk_rows - 1) // chunk_rows
    arenas = {"x": Arena(rows, C0, "elem", ld=C0 + pad, col_off=pad, poison="nan", data=rnd((rows, C0), 1) + 0.5),
              "x1": Arena(rows, C1, "elem", ld=C1 + pad, col_off=pad, poison="nan", data=2.0 * rnd((rows, C1), 2)),
              "part": Arena(nstat * nchunk, 64, "f32", tile=(1, 64))}
    if form == "table":
        arenas["y"] = Arena(nstat * 2, Cc, "f32", tile=(2, Cc))
        silu = False
    else:
        arenas["y"] = Arena(rows, Cc, "elem", ld=Cc + pad, col_off=pad, tile=(rps, Cc))
    dn = {"gamma": 1 + 0.1 * rnd((Cc,), 3), "beta": 0.1 * rnd((Cc,), 4)}
    cols = ops.gn_fused_cols(rps, Cc) if form == "fused" else 0
    assert form != "fused" or cols > 0

    def build(b):
        return ops.gn_params(b["x"], C0 + pad, C0, rows, rps, b["part"], b["gamma"], b["beta"], 1e-5, silu, b["y"], Cc + pad if form != "table" else Cc,
                             x1=b["x1"], ld1=C1 + pad, C1=C1, chunk_rows=cols if form == "fused" else chunk_rows)

    def ref(p):
        if form == "fused":
            return I.groupnorm_fused(p)
        I.groupnorm_stats(p)
        (I.groupnorm_table if form == "table" else I.groupnorm)(p)

    def gpu(lib, p, st):
        if form == "fused":
            return lib.vmv_groupnorm_fused(C.byref(p), cols, st)
        rc = lib.vmv_groupnorm_stats(C.byref(p), st)
        return rc or (lib.vmv_groupnorm_table if form == "table" else lib.vmv_groupnorm_apply)(C.byref(p), st)

    tol = {} if form == "table" else dict(tol_l2=5e-3, tol_max=2e-2 if form == "fused" else 1.5e-2)
    return FCase(f"groupnorm[{form}]", arenas, dn, build, ref, gpu, {"y": tol})


# ------------------------------------------------------------------------------------------------- attention
ATTN_CASES = {"spatial": ("spatial", 1, 2, 16, 5), "cross": ("cross", 2, 3, 64, 2), "temporal": ("temporal", 1, 4, 9, 1), "causal": ("causal", 1, 77, 1, 2),
              "hd32": ("hd32", 1, 130, 1, 3)}


def attention_case(key, dense=False):
    """vmv_attention with the output written through `om` into a wider row (s_row = inner + 64), the head slices at a column offset; q | k | v
    read as slices of padded rows; guard rows after the last problem.  The smallest existing test shape of each form."""
    kind, B, F_, HW, heads = ATTN_CASES[key]
    hd = 32 if kind == "hd32" else 64
    inner = heads * hd
    Lc = 77
    opad, ooff = (0, 0) if dense else (64, 32)
    ipad = 0 if dense else 8
    if kind in ("causal", "hd32"):
        B, T = B, F_              # (B, T, -, heads): one problem per batch item, T tokens
        F_, HW = 1, T
    T = B * F_ * HW
    lo = inner + opad
    arenas = {"o": Arena(T, inner, "elem", ld=lo, col_off=ooff, tile=(64, hd))}
    if kind == "cross":
        arenas["q"] = Arena(T, inner, "elem", ld=inner + ipad, col_off=ipad, poison="nan", data=rnd((T, inner), 1))
        arenas["kv"] = Arena(B * Lc, 2 * inner, "elem", ld=2 * inner + ipad, col_off=ipad, poison="nan", data=rnd((B * Lc, 2 * inner), 2))
    else:
        arenas["qkv"] = Arena(T, 3 * inner, "elem", ld=3 * inner + ipad, col_off=ipad, poison="nan", data=rnd((T, 3 * inner), 5))

    def build(b):
        sc = hd ** -0.5
        if kind == "temporal":
            mp = lambda ld: ops.seq_map(F_ * HW * ld, ld, HW * ld, inner=HW)
            n_outer, Nq = B * HW, F_
        else:
            mp = lambda ld: ops.seq_map(HW * ld, 0, ld, inner=1)
            n_outer, Nq = B * F_, HW
        if kind == "cross":
            lkv = 2 * inner + ipad
            kvm = ops.seq_map(Lc * lkv, 0, lkv, inner=1)
            return ops.attn_params(b["q"], b["kv"], b["kv"] + 2 * inner, b["o"], mp(inner + ipad), kvm, kvm, mp(lo), n_outer, heads, Nq, Lc, sc, kv_div=F_)
        ld = 3 * inner + ipad
        base = b["qkv"]
        return ops.attn_params(base, base + 2 * inner, base + 4 * inner, b["o"], mp(ld), mp(ld), mp(ld), mp(lo), n_outer, heads, Nq, Nq, sc, head_dim=hd,
                               causal=kind == "causal")

    return FCase(f"attention[{key}]", arenas, {}, build, I.attention, lambda lib, p, st: lib.vmv_attention(C.byref(p), st), {"o": dict(tol_l2=6e-3, tol_max=2e-2)})


# ------------------------------------------------------------------------------------------------- glue kernels
def _glue(name, arenas, dense, ref, gpu, outs):
    return FCase(name, arenas, dense, lambda b: b, ref, gpu, outs)


def avgpool_case():
    n, Cc, IH, IW, OH, OW = 2, 32, 9, 14, 4, 4
    a = {"x": Arena(n * IH * IW, Cc, "elem", ld=Cc + 8, col_off=8, poison="nan", data=rnd((n * IH * IW, Cc), 3)),
         "y": Arena(n * OH * OW, Cc, "elem", ld=Cc + 8, col_off=8)}
    return _glue("adaptive_avgpool_rows", a, {}, lambda b: I.adaptive_avgpool_rows(b["x"], Cc + 8, b["y"], Cc + 8, n, Cc, IH, IW, OH, OW),
                 lambda lib, b, st: lib.vmv_adaptive_avgpool_rows(b["x"], Cc + 8, b["y"], Cc + 8, n, Cc, IH, IW, OH, OW, st), {"y": dict(tol_l2=4e-3, tol_max=1e-2)})


def i2v_adapter_case():
    """channels 4..7 of 16-wide rows are written (out = base + 4), everything else of the row is guard"""
    F_, HW, nrep = 6, 11, 2
    w = 0.5 * rnd((288,), 2)
    w[0:4] = 1 + 0.1 * w[0:4]
    a = {"x": Arena(F_ * HW, 4, "elem", ld=8, col_off=4, poison="nan", data=rnd((F_ * HW, 4), 1)), "y": Arena(nrep * F_ * HW, 4, "elem", ld=16, col_off=4)}
    return _glue("i2v_temporal_adapter", a, {"w": w}, lambda b: I.i2v_temporal_adapter(b["x"], 8, b["y"], 16, b["w"], F_, HW, nrep, 2.0),
                 lambda lib, b, st: lib.vmv_i2v_temporal_adapter(b["x"], 8, b["y"], 16, b["w"].data_ptr(), F_, HW, nrep, 2.0, st),
                 {"y": dict(tol_l2=5e-3, tol_max=1.5e-2)})


def latent_to_rows_case(keep):
    """vmv_latent_to_rows writes whole Cpad-wide rows (dense by contract: guard rows around them); _keep writes channels [0, C) of ld-wide rows"""
    nb, Cc, F_, H, W, nrep = 1, 4, 3, 5, 6, 2
    rows = nrep * nb * F_ * H * W
    a = {"rows": Arena(rows, Cc, "elem", ld=16, col_off=0) if keep else Arena(rows, 8, "elem", ld=8)}
    dn = {"lat": rnd((nb, Cc, F_, H, W), 4)}

    def ref(b):
        whole = b.buf("rows").view(-1, a["rows"].ld)[G_BEFORE:G_BEFORE + rows]
        (I.latent_to_rows_keep(b["lat"], whole, 16, nrep) if keep else I.latent_to_rows(b["lat"], whole, 8, nrep))

    def gpu(lib, b, st):
        if keep:
            return lib.vmv_latent_to_rows_keep(b["lat"].data_ptr(), b["rows"], nb, Cc, F_, H, W, 16, nrep, st)
        return lib.vmv_latent_to_rows(b["lat"].data_ptr(), b["rows"], nb, Cc, F_, H, W, 8, nrep, st)

    return _glue("latent_to_rows_keep" if keep else "latent_to_rows", a, dn, ref, gpu, {"rows": "exact"})


def rows_to_nchw_case():
    """source rows with a padded stride (NaN around the C channels read), the dense [n][C][HW] fp32 destination between guard rows"""
    n, Cc, H, W = 3, 4, 6, 7
    a = {"rows": Arena(n * H * W, Cc, "f32", ld=12, col_off=4, poison="nan", data=rnd((n * H * W, Cc), 3)), "out": Arena(n * Cc, H * W, "f32")}

    def ref(b):
        b.payload("out").copy_(b.payload("rows").reshape(n, H * W, Cc).permute(0, 2, 1).reshape(n * Cc, H * W))

    return _glue("rows_to_nchw", a, {}, ref, lambda lib, b, st: lib.vmv_rows_to_nchw(b["rows"], 1, 12, b["out"], n, Cc, H * W, st), {"out": "exact"})


def emb_combine_case():
    rows, Cc, rpt, cam_rows = 10, 40, 5, 5
    a = {"out": Arena(rows, Cc, "elem")}
    dn = {"temb": rnd((rows // rpt, Cc), 1), "cam": rnd((cam_rows, Cc), 2)}
    return _glue("emb_combine_silu", a, dn, lambda b: I.emb_combine_silu(b["temb"], b["cam"], b.payload("out"), rows, Cc, rpt, cam_rows),
                 lambda lib, b, st: lib.vmv_emb_combine_silu(b["temb"].data_ptr(), b["cam"].data_ptr(), b["out"], rows, Cc, rpt, cam_rows, st),
                 {"out": dict(tol_l2=4e-3, tol_max=1e-2)})


def permute_copy_case():
    """send[s][bf][p c] <- x[bf][s][p c] with padded source strides: every (bf, s) block of the source is followed by 16 pad bytes (NaN)"""
    R, BF_, Pl, Cc = 4, 6, 10, 64
    inner16 = Pl * Cc // 8
    blk = inner16 + 1                           # source block stride in 16-byte units: one vector of pad per block
    a = {"src": Arena(BF_ * R, inner16 * 8, "elem", ld=blk * 8, poison="nan", data=rnd((BF_ * R, inner16 * 8), 7)), "dst": Arena(R * BF_, inner16 * 8, "elem")}

    def build(b):
        return ops.copy_params(b["src"], b["dst"], R, BF_, 1, inner16, blk, R * blk)

    return FCase("permute_copy", a, {}, build, I.permute_copy, lambda lib, p, st: lib.vmv_permute_copy(C.byref(p), st), {"dst": "exact"})


def _whole(b, k):
    """[rows][ld] host view of arena k from the kernel's pointer (col_off = 0)"""
    a = b.case.arenas[k]
    return b.buf(k).view(-1, a.ld)[a.gb:a.gb + a.rows]


F32_TOL = dict(tol_l2=1e-3, tol_max=2e-3)          # fp32 in, fp32 out: as the fp32-output GEMM cases (the fp64 comparison is tests/test_glue_gpu.py)


def cfg_ddim_case():
    """eps rows of stride C + 4 (NaN pad); xt (in place), x0_out and noise dense [C][F * HW] between guard rows; clamp and sigma > 0"""
    Cc, F_, HW = 4, 3, 37
    FHW, ld = F_ * HW, Cc + 4
    kw = dict(guide_scale=9.0, c_recip=1.31, c_recipm1=0.85, c_sqrt_ac=0.76, c_sqrt_1mac=0.65, a_prev=0.71, clamp=1.1, sigma=0.2)
    a = {"eps": Arena(2 * FHW, Cc, "f32", ld=ld, poison="nan", data=rnd((2 * FHW, Cc), 2)), "xt": Arena(Cc, FHW, "f32", data=rnd((Cc, FHW), 1)),
         "x0": Arena(Cc, FHW, "f32"), "noise": Arena(Cc, FHW, "f32", poison="nan", data=rnd((Cc, FHW), 5))}
    sh = (1, Cc, F_, 1, HW)

    def ref(b):
        I.cfg_ddim_step(_whole(b, "eps"), ld, b.payload("xt").view(sh), x0_out=b.payload("x0").view(sh), noise=b.payload("noise").view(sh), **kw)

    def gpu(lib, b, st):
        p = L.DdimParams()
        p.eps_rows, p.ld, p.C, p.F, p.HW = b["eps"], ld, Cc, F_, HW
        p.guide_scale, p.c_recip, p.c_recipm1, p.c_sqrt_ac, p.c_sqrt_1mac, p.a_prev, p.v_pred = 9.0, 1.31, 0.85, 0.76, 0.65, 0.71, 0
        p.xt, p.x0_out, p.clamp, p.sigma, p.noise = b["xt"], b["x0"], 1.1, 0.2, b["noise"]
        return lib.vmv_cfg_ddim_step(C.byref(p), st)

    return _glue("cfg_ddim_step", a, {}, ref, gpu, {"xt": F32_TOL, "x0": F32_TOL})


def ddim_x0_case():
    """xt updated in place between guard rows"""
    n = 445
    u = rnd((n,), 1)
    a = {"xt": Arena(1, n, "f32", data=rnd((1, n), 3))}
    dn = {"c": u + 0.3 * rnd((n,), 2), "u": u, "noise": rnd((n,), 4)}
    args = (9.0, 1.31, 0.85, 0.71)
    return _glue("ddim_x0_step", a, dn, lambda b: I.ddim_x0_step(b["c"], b["u"], b.payload("xt").view(n), *args, clamp=1.1, sigma=0.2, noise=b["noise"]),
                 lambda lib, b, st: lib.vmv_ddim_x0_step(b["c"].data_ptr(), b["u"].data_ptr(), b["xt"], n, *args, 1.1, 0.2, b["noise"].data_ptr(), st), {"xt": F32_TOL})


def posterior_case():
    """moments rows of stride 2 zc + 4 (NaN pad)"""
    n, zc, HW = 2, 4, 37
    ld = 2 * zc + 4
    mom = torch.cat([rnd((n * HW, zc), 1), 3.0 * rnd((n * HW, zc), 2)], dim=1)
    a = {"mom": Arena(n * HW, 2 * zc, "f32", ld=ld, poison="nan", data=mom), "z": Arena(n * zc, HW, "f32")}
    dn = {"noise": rnd((n, zc, 1, HW), 3)}
    return _glue("posterior_sample", a, dn, lambda b: I.posterior_sample(_whole(b, "mom"), ld, b["noise"], b.payload("z").view(n, zc, 1, HW), 0.18215),
                 lambda lib, b, st: lib.vmv_posterior_sample(b["mom"], ld, b["noise"].data_ptr(), b["z"], n, zc, HW, 0.18215, st), {"z": F32_TOL})


def lgm_x0_views_case():
    """eps rows of stride C + 4; NaN in the pad, in the frames idx4 does not name (eps and xt) and in the whole other branch"""
    Cc, F_, HW, branch, idx4 = 4, 5, 37, 1, (4, 0, 2, 2)
    ld = Cc + 4
    eps = rnd((2, F_, HW, Cc), 1)
    xt = rnd((1, Cc, F_, 1, HW), 2)
    eps[1 - branch] = float("nan")
    for f in range(F_):
        if f not in idx4:
            eps[:, f], xt[:, :, f] = float("nan"), float("nan")
    a = {"eps": Arena(2 * F_ * HW, Cc, "f32", ld=ld, poison="nan", data=eps.reshape(-1, Cc)), "out": Arena(4 * Cc, HW, "f32")}
    ia = (C.c_int32 * 4)(*idx4)
    return _glue("lgm_x0_views", a, {"xt": xt},
                 lambda b: I.lgm_x0_views(_whole(b, "eps"), ld, branch, b["xt"], idx4, 1.31, 0.85, 5.49, b.payload("out").view(4, Cc, 1, HW)),
                 lambda lib, b, st: lib.vmv_lgm_x0_views(b["eps"], ld, branch, b["xt"].data_ptr(), Cc, F_, HW, ia, 1.31, 0.85, 5.49, b["out"], st), {"out": F32_TOL})


def lgm_pack_input_case():
    V, HW = 3, 37
    a = {"dec": Arena(V * 3, HW, "f32", poison="nan", data=rnd((V * 3, HW), 1, 1.2)), "rays": Arena(V * 6, HW, "f32", poison="nan", data=rnd((V * 6, HW), 2)),
         "out": Arena(V * 9, HW, "f32")}
    return _glue("lgm_pack_input", a, {},
                 lambda b: I.lgm_pack_input(b.payload("dec").view(V, 3, 1, HW), b.payload("rays").view(V, 6, 1, HW), b.payload("out").view(V, 9, 1, HW)),
                 lambda lib, b, st: lib.vmv_lgm_pack_input(b["dec"], b["rays"], b["out"], V, HW, st), {"out": F32_TOL})


def gaussian_activation_case():
    """raw rows of stride 16 with NaN in columns 14 and 15; the workspace is guarded beyond its 4 floats per first-pass block"""
    n = 600
    blocks = (n + 255) // 256
    a = {"raw": Arena(n, 14, "f32", ld=16, poison="nan", data=2.0 * rnd((n, 14), 11)), "out": Arena(n, 14, "f32"), "ws": Arena(1, 4 * blocks, "f32")}
    return _glue("gaussian_activation", a, {}, lambda b: I.gaussian_activation(_whole(b, "raw"), 16, b.payload("out"), n, None),
                 lambda lib, b, st: lib.vmv_gaussian_activation(b["raw"], 16, b["out"], n, b["ws"], st), {"out": F32_TOL})


GLUE = {"adaptive_avgpool_rows": avgpool_case, "i2v_temporal_adapter": i2v_adapter_case, "latent_to_rows": lambda: latent_to_rows_case(False),
        "latent_to_rows_keep": lambda: latent_to_rows_case(True), "rows_to_nchw": rows_to_nchw_case, "emb_combine_silu": emb_combine_case,
        "permute_copy": permute_copy_case, "cfg_ddim_step": cfg_ddim_case, "ddim_x0_step": ddim_x0_case, "posterior_sample": posterior_case,
        "lgm_x0_views": lgm_x0_views_case, "lgm_pack_input": lgm_pack_input_case, "gaussian_activation": gaussian_activation_case}
