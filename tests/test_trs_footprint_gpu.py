"""The store footprint of the row-stationary temporal convolution (csrc/gemm_trs.hip) at one ragged shape — `pytest -m gpu`.

Harness and checks are those of tests/footprint.py / tests/test_footprint_gpu.py (arenas: the output between guard rows and guard columns
that must keep their bit pattern, the source and the residual between NaN; the payload against the interpreter and, bit for bit, against
the same launch on dense buffers).  Two samples of 11 pixels at F = 24: 22 (sample, pixel) indices = one full row tile of 16 and a second
one with three waves of pixels and five of padding; the seam between the samples lies inside a wave.  Folded GroupNorm + SiLU, residual
with its own row pitch, every operand 8 columns into rows 8 (16) wider than its payload.
"""
import ctypes as C

import pytest
import torch

from videomv_amd import _lib as L
from videomv_amd import ops
from tests import footprint as FP
from tests import plan_interp as I
from tests.test_footprint_gpu import run_case

pytestmark = pytest.mark.gpu


def trs_case(dense=False):
    Bn, F_, Pp, Cc, N = 2, 24, 11, 320, 320
    M = Bn * F_ * Pp
    pad = not dense
    arenas = {"x0": FP.Arena(M, Cc, "elem", ld=Cc + 8 if pad else Cc, col_off=8 if pad else 0, g_before=FP.G_SRC, poison="nan", data=FP.rnd((M, Cc), 11) + 0.3)}
    dn = {"w": FP.rnd((N + 512, 3 * Cc), 2, (3 * Cc) ** -0.5).to(L.elem()), "bias": FP.rnd((N + 512,), 3),
          "tab": torch.stack([1 + 0.2 * FP.rnd((Bn + 2, Cc), 8), 0.1 * FP.rnd((Bn + 2, Cc), 9)], dim=1).contiguous()}
    ldo, ooff = (N + 16, 8) if pad else (N, 0)
    arenas["out"] = FP.Arena(M, N, "elem", ld=ldo, col_off=ooff, tile=(48, 64))
    arenas["res"] = FP.Arena(M, N, "elem", ld=N + 8 if pad else N, col_off=8 if pad else 0, poison="nan", data=FP.rnd((M, N), 5))

    def build(b):
        return ops.gemm_params(M, N, ops.temporal_segs(b["x0"], arenas["x0"].ld, Cc), b["w"], b["out"], ldo, bias=b["bias"], geom=ops.Geom(F=F_, P=Pp),
                               residual=b["res"], ldr=arenas["res"].ld, gn_table=b["tab"], gn_rows_per_stat=F_ * Pp, gn_silu=True, tile=L.TRS_TILE)

    return FP.FCase(f"gemm[TRS-l-silu-res{'-dense' if dense else ''}]", arenas, dn, build, I.gemm, lambda lib, p, st: lib.vmv_gemm(C.byref(p), st),
                    {"out": dict(tol_l2=6e-3, tol_max=2.5e-2)}, tile=L.TRS_TILE)


def test_trs_footprint():
    lib = L.load()
    case = trs_case()
    p = case.build(case.on("cpu"))
    assert lib.vmv_gemm_validate(C.byref(p)) == 0 and lib.vmv_gemm_served_tile(C.byref(p)) == L.TRS_TILE
    run_case(case, trs_case(dense=True))
