"""GPU matrix of vmv_attention — `pytest -m gpu`: every dispatch branch against the fp64 reference of tests/attn_ref.py.

Every case (the literal table attn_ref.GPU_CASES) 1. asserts vmv_attention_served_kernel names the branch the case is there for, 2. runs
the kernel through ops.Stream(record=False).attention into a zeroed output (a tile that is never computed shows), 3. compares EVERY
problem with the reference under the project's attention bound, check(tol_l2=6e-3, tol_max=2e-2) x TS (TS = 1 for bf16, 0.125 for
fp16), and 4. runs once more into a fresh output and asserts the two are bitwise equal.  Inputs come from the score profiles of
attn_ref.patterns: the sinks, ramps and single climbing queries that select the kernels' rescale / rescale-skip paths and, in the
fp16 build, make the tail of P a subnormal MFMA operand (tests/test_attention_cpu.py shows that a flushed tail breaks this bound).
Each test prints its figures before it asserts."""
import ctypes as C

import pytest
import torch

from videomv_amd import _lib as L
from videomv_amd import ops
from tests import attn_ref as R

pytestmark = pytest.mark.gpu

# profile, G: sinks at 10 and 14, ramps at 14, scores spanning +-60
FULL = [("random", 0.0), ("uniform", 0.0), ("early_sink", 10.0), ("early_sink", 14.0), ("late_sink", 10.0), ("late_sink", 14.0),
        ("ramp_up", 14.0), ("ramp_down", 14.0), ("one_query", 14.0), ("large", 60.0)]
# one case of each branch with at least three key tiles carries the full list; SHORT (one tile, no rescale) the P rounding and masked-key paths
PROFILED = {"wave_4x2_24x130": FULL, "q128_64x4096": FULL, "q256_512": FULL, "q256_2100x577": FULL, "d32_130": FULL, "d128_129": FULL,
            "causal_129": [("random", 0.0), ("ramp_up", 14.0), ("one_query", 14.0), ("large", 60.0)],
            "short_7x2_17x31": [("random", 0.0), ("early_sink", 10.0), ("early_sink", 14.0), ("late_sink", 10.0), ("late_sink", 14.0), ("large", 60.0)],
            "short_5x3_32x32": [("random", 0.0), ("early_sink", 14.0), ("late_sink", 14.0), ("large", 60.0)]}
MATRIX = [(c[0], prof, G) for c in R.GPU_CASES for prof, G in PROFILED.get(c[0], [("random", 0.0)])]


def _run(c, dev):
    """served kernel == the case's branch; launch into dev['o']; launch again into a fresh zeroed output: bitwise equal.  Returns params."""
    branch = R.CASE_BY_NAME[c.name][1]
    p = c.build(dev)
    assert L.load().vmv_attention_served_kernel(C.byref(p)) == R.branch_id(branch), (c.name, branch)
    assert float(dev["o"].float().abs().max()) == 0.0
    S = ops.Stream(record=False)
    S.attention(p, c.name)
    again = dict(dev, o=torch.zeros_like(dev["o"]))
    S.attention(c.build(again), c.name)
    torch.cuda.synchronize()
    assert torch.equal(dev["o"].view(torch.int16), again["o"].view(torch.int16)), "two runs of the same launch differ"
    return p


def _case(name, profile="random", G=0.0, seed=7):
    c = R.case(name).fill(profile, G, seed)
    c.name = name
    return c


@pytest.mark.parametrize("name,profile,G", MATRIX, ids=[f"{n}-{pr}{int(G) if G else ''}" for n, pr, G in MATRIX])
def test_attention_matrix(name, profile, G):
    c = _case(name, profile, G)
    dev = c.on("cuda")
    p = _run(c, dev)
    bufs = list(dev.values())
    ref = R.reference(p, bufs)                                   # fp64 on the device, every problem
    out = R.gather(p, "o", bufs)
    assert torch.equal(out, c.logical_out(dev["o"]))
    e_l2, e_max = R.errors(out, ref)
    tol_l2, tol_max = R.bound(c.dtype)
    print(f"ATTN_ERR {R.CASE_BY_NAME[name][1]} {L.elem_name()} {name} {profile} {G:g} rel-L2 {e_l2:.3e} max {e_max:.3e} (bound {tol_l2:.2e} / {tol_max:.2e})")
    assert e_l2 < tol_l2 and e_max < tol_max, (e_l2, e_max, tol_l2, tol_max)
    if c.hd == 128:                                              # the zero padding of the 80-wide heads stays exactly zero
        assert float(out[..., 80:].float().abs().max()) == 0.0


@pytest.mark.parametrize("name", ["short_32x1", "q128_100x1", "d32_70x1", "d128_40x1"])
def test_attention_single_key_returns_v_bit_for_bit(name):
    """Nk = 1: P = exp2(0) = 1, l = 1, the masked keys of the tile contribute exactly 0 — every output row is V's row of its problem and head."""
    c = _case(name)
    dev = c.on("cuda")
    p = _run(c, dev)
    bufs = list(dev.values())
    out, v = R.gather(p, "o", bufs), R.gather(p, "v", bufs)      # [problem][head][Nq][d], [problem][head][1][d]
    assert torch.equal(out.view(torch.int16), v.expand_as(out).contiguous().view(torch.int16))


@pytest.mark.parametrize("name", ["wave_4x2_24x130", "q128_64x4096", "q256_512"])
def test_attention_uniform_scores_average_v_to_one_ulp(name):
    """q = 0: every P is exactly 1 and l exactly Nk, so the output is the mean of V (U[1, 2)) up to the fp32 accumulation of <= 4096 terms
    (about 1e-6 relative, far below the element's half-ulp): within one unit in the last place of the fp64 mean rounded to the element type."""
    c = _case(name, "uniform")
    dev = c.on("cuda")
    p = _run(c, dev)
    bufs = list(dev.values())
    out = R.gather(p, "o", bufs)
    mean = R.gather(p, "v", bufs).double().mean(dim=2, keepdim=True).to(c.dtype)
    assert 1.0 <= float(mean.float().min()) and float(mean.float().max()) <= 2.0      # one binade: a difference of the bit patterns counts ulps
    ulps = (out.view(torch.int16).int() - mean.view(torch.int16).int().expand_as(out)).abs()
    print(f"ATTN_ULP {R.CASE_BY_NAME[name][1]} {L.elem_name()} {name} max {int(ulps.max())} ulp, {float((ulps == 0).float().mean()):.4f} exact")
    assert int(ulps.max()) <= 1
