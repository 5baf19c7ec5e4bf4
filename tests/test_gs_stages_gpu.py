"""The Gaussian rasteriser's forward pass on the device, STAGE BY STAGE (csrc/raster.hip + gs_common.h through GaussianRenderer.render,
VMV_GS_BATCH=0, render_depth and GaussianFitter._forward) against tests/gs_stage_ref.py (checked without a GPU in
tests/test_gs_stages_cpu.py).  After each render the arrays the kernels left on the device (``GaussianRenderer.binning`` /
``binning_view``) are read back and held to
  (a) preprocess  the fp64 reference: culled / valid, tiles_touched and rect EXACT away from boundary records, a neighbouring decision on
                  them; xy, conic and depth of the valid records within 8 x the fp32 oracle's own distance from the fp64 reference;
  (b) binning     exact, both key forms: ranges, sorted keys, every tile's slice of the sorted values in (depth bits, index) order;
  (c) blend       every non-ambiguous pixel, no share allowance: n_contrib exact, the median's Gaussian exact, image / alpha / final T /
                  expected depth per pixel within max(2e-5, 8 x the error of an fp32 CPU evaluation of the same reference);
and the four paths give the same bits.

Cases (tests/gs_stage_ref.py CASES; B, V, N, S) and what each pins:
  plain        1, 3, 300, 64    baseline; V N = 900 is no multiple of 256
  partial-40   2, 2, 200, 40    size % 16 != 0 (grid 3, 8-pixel edge tiles) and the sample offset of ``gaussians``;  partial-50: 1, 1, 200, 50
  dup-256/257/255/span  1, 2, 128, 32 / 1, 1, 257, 32 / 1, 3, 85, 32 / 1, 3, 100, 32    a 256-rank duplicate block exactly full, one record
               into the next, one short, and a block spanning two views
  rounds       1, 2, 64, 272    289 tiles; 24 Gaussians that touch more than 256 of them (one owner over several 256-slot rounds) between
               40 culled records (equal offsets in the owner search), the first and the last record among them
  ties         1, 2, 96, 48     32 positions used three times: equal depth bits blend in index order on both paths
  empty-views  1, 4, 100, 32    views 1 and 3 see nothing: a duplicate block without instances, ranges of an empty view inside and last
  bits-17/32/1/9  (1, 17, 40, 16), (1, 2, 60, 64), (1, 1, 40, 16), (1, 1, 60, 48)    V x tiles = 2^4 + 1, 2^5, 1, 9: the highest tile id sorts last
  deep-900/511/512/513  1, 1, n, 32    one tile list longer than three LDS chunks; chunk tails odd, full and lone in the forward and depth blends
  stop         1, 2, 200, 32    dense opaque cluster: pixels stop before T < 1e-4, n_contrib ends before the stopping Gaussian

MEASURED on an MI355X (largest figure over all 19 cases and their views; the test prints them per case and view).  No comparator failed:
no kernel or host fix was called for, and no bound was moved.
  quantity                       kernel vs fp64    held against
  xy (px)                        1.34e-05          8 x fp32 oracle vs fp64: 1.34e-05 (both in "rounds", S = 272; 1.2e-06 .. 8.7e-06 elsewhere)
  conic (relative)               1.87e-06          8 x fp32 oracle vs fp64: 1.20e-06 ("ties"; 1.9e-07 .. 8.1e-07 against 2.5e-07 .. 8.6e-07 elsewhere)
  depth (relative)               9.14e-08          8 x fp32 oracle vs fp64: 9.14e-08 (equal to the oracle's in 17 cases, below it in 2)
  culled / tiles_touched / rect  exact             away from boundary records; on them a neighbouring decision
  binning, n_contrib, median     exact             0 pixels differ
  image                          4.25e-07          max(2e-5, 8 x fp32 CPU evaluation vs fp64: 4.25e-07): the 2e-5 floor binds everywhere
  alpha                          6.67e-07          max(2e-5, 8 x 2.54e-07)
  final T                        2.33e-07          max(2e-5, 8 x 2.66e-07)
  expected depth / z_max         5.87e-07          max(2e-5, 8 x 2.19e-07)
The v_exp_f32 / v_log_f32 path therefore costs at most 3 x the fp32 CPU evaluation's error per pixel, 30 x below the floor.
Excluded shares seen: boundary records 0 % in 14 cases, else 0.22 % (deep-900), 0.29 % (bits-17), 0.33 % (plain), 0.38 % (partial-40),
0.75 % (empty-views); ambiguous pixels per view 0 .. 0.39 % (largest: bits-17 and bits-1, one pixel of 256); ambiguous medians per view
0 .. 0.78 % (largest: dup-257 and stop, 8 pixels of 1024).
"""
import functools

import pytest
import torch

from oracle.gs_ref import preprocess
from tests import gs_stage_ref as R

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _reference(name):
    """the case, the fp64 preprocess reference of every view and the fp32 oracle's own distance from it: computed once, never modified"""
    g, cv, cvp, S = R.build_case(name)
    refs, oracle = [], dict(xy=0.0, conic=0.0, depth=0.0)
    for b in range(g.shape[0]):
        for v in range(cv.shape[1]):
            ref = R.preprocess_ref(g[b], cv[b, v], cvp[b, v], S)
            pp = preprocess(g[b, :, 0:3], g[b, :, 4:7], g[b, :, 7:11], cv[b, v], cvp[b, v], S, R.TAN)
            err = R.preprocess_errors(ref, pp["depth"], pp["xy"], pp["conic"], pp["valid"] & ref["valid"])
            oracle = {k: max(oracle[k], err[k]) for k in oracle}
            refs.append(ref)
    return g, cv, cvp, S, refs, oracle


_read = R.read_arrays


def _same_preprocess(a, b, label):
    """two passes over the same inputs leave the same bits in the records that touch a tile (the others keep what they held)"""
    assert torch.equal(a["tiles_touched"], b["tiles_touched"]), label
    m = a["tiles_touched"] > 0
    for k in ("depth", "xy", "conic_opacity", "rect"):
        assert torch.equal(a[k][m], b[k][m]), (label, k)


def _check_binning(a, S, label):
    lists = R.binning_ref(a["tiles_touched"], a["rect"], R.depth_bits(a["depth"]), S)
    R.check_binning(lists, a["tiles_touched"], a["ranges"], a["vals_sorted"], a["keys_sorted"], a["n"], R.depth_bits(a["depth"]), label)
    return lists


@pytest.mark.parametrize("name", list(R.CASES))
def test_stages(name, monkeypatch):
    from videomv_amd.gs import GaussianRenderer
    from videomv_amd.gs_fit import GaussianFitter
    g, cv, cvp, S, refs, oracle = _reference(name)
    B, V, N = g.shape[0], cv.shape[1], g.shape[1]
    tiles = ((S + 15) // 16) ** 2
    gd, cvd, cvpd, bg = g.cuda(), cv.cuda(), cvp.cuda(), torch.tensor(R.BG)
    r = GaussianRenderer(S, R.FOVY)
    monkeypatch.setenv("VMV_GS_BATCH", "1")
    out = r.render(gd, cvd, cvpd, None, bg_color=bg)
    a = _read(r.binning(B, V, N, gd.device))
    assert r.last_num_rendered == [a["n"]]

    # (a) preprocess against fp64
    kernel = dict(xy=0.0, conic=0.0, depth=0.0)
    boundary = sum(int(ref["boundary"].sum()) for ref in refs) / (B * V * N)
    assert boundary <= R.BOUNDARY_CAP, boundary
    for vv, ref in enumerate(refs):
        R.check_preprocess(ref, a["tiles_touched"][vv], a["rect"][vv], S, f"{name} view {vv}")
        err = R.preprocess_errors(ref, a["depth"][vv], a["xy"][vv], a["conic_opacity"][vv, :, :3], (a["tiles_touched"][vv] > 0) & ref["valid"])
        kernel = {k: max(kernel[k], err[k]) for k in kernel}
        m = a["tiles_touched"][vv] > 0
        assert torch.equal(a["conic_opacity"][vv, :, 3][m], g[vv // V, :, 3][m])
    print(f"gs stages {name}: boundary records {boundary:.3%}; kernel vs fp64 " + ", ".join(f"{k} {v:.3e}" for k, v in kernel.items())
          + "; fp32 oracle vs fp64 " + ", ".join(f"{k} {v:.3e}" for k, v in oracle.items()))
    for k in kernel:
        assert kernel[k] <= 8.0 * oracle[k], (k, kernel[k], oracle[k])

    # (b) binning, exact (batched form)
    lists = _check_binning(a, S, f"{name} batched")

    # the other three paths: the same preprocess bits, their own binning exact, the same image bits
    outd = r.render_depth(gd, cvd, cvpd, None, bg_color=bg)
    ad = _read(r.binning(B, V, N, gd.device))
    _same_preprocess(a, ad, "depth mode")
    _check_binning(ad, S, f"{name} depth mode")
    assert torch.equal(outd["image"], out["image"]) and torch.equal(outd["alpha"], out["alpha"])
    f = GaussianFitter(gd, cvd, cvpd, torch.zeros(B, V, 3, S, S).cuda(), bg=R.BG, fovy=R.FOVY)
    f.gs.copy_(gd.reshape(-1, 14))                          # the Gaussians exactly as given (raw quaternions)
    f._forward()
    af = _read(f.renderer.binning(B, V, N, gd.device))
    _same_preprocess(a, af, "forward with state")
    _check_binning(af, S, f"{name} forward with state")
    assert f.num_rendered == a["n"]
    assert torch.equal(f.image.reshape(out["image"].shape), out["image"]) and torch.equal(f.alpha.reshape(out["alpha"].shape), out["alpha"])
    monkeypatch.setenv("VMV_GS_BATCH", "0")
    for b in range(B):
        for v in range(V):
            one = r.render(gd[b:b + 1], cvd[b:b + 1, v:v + 1].contiguous(), cvpd[b:b + 1, v:v + 1].contiguous(), None, bg_color=bg)
            av = _read(r.binning_view(N, gd.device))
            vv = b * V + v
            assert av["keys_sorted"].dtype == torch.int64 and r.last_num_rendered == [av["n"]]
            _same_preprocess({k: a[k][vv:vv + 1] for k in ("tiles_touched", "depth", "xy", "conic_opacity", "rect")}, av, f"per-view {vv}")
            mine = _check_binning(av, S, f"{name} per-view {vv}")
            assert all(torch.equal(x, y) for x, y in zip(mine, lists[vv * tiles:(vv + 1) * tiles]))
            assert torch.equal(one["image"][0, 0], out["image"][b, v]) and torch.equal(one["alpha"][0, 0], out["alpha"][b, v])

    # (c) blend against the fp64 blend over the kernel's own lists and preprocess arrays, per pixel
    cpu = lambda t: t.cpu()
    image, alpha, depth, median = (cpu(x).reshape(B * V, -1, S, S) for x in (out["image"], out["alpha"], outd["depth"], outd["median_depth"]))
    final_T, n_contrib = cpu(f.final_T), cpu(f.n_contrib)
    stops = 0
    for vv in range(B * V):
        args = (lists[vv * tiles:(vv + 1) * tiles], a["xy"][vv], a["conic_opacity"][vv], g[vv // V, :, 11:14], a["depth"][vv], S, R.BG)
        ref, ref32 = R.blend_ref(*args), R.blend_ref(*args, dtype=torch.float32)
        m = a["tiles_touched"][vv] > 0
        z_max = float(a["depth"][vv][m].max()) if bool(m.any()) else 1.0
        bounds, err32 = R.blend_bounds(ref, ref32, z_max)
        print(f"gs stages {name} view {vv}: fp32 CPU evaluation vs fp64 " + ", ".join(f"{k} {v:.3e}" for k, v in err32.items()))
        R.check_blend(ref, bounds, z_max, f"{name} view {vv}", image=image[vv], alpha=alpha[vv, 0], T=final_T[vv], depth=depth[vv, 0],
                      median=median[vv, 0], n_contrib=n_contrib[vv])
        if not bool(m.any()):                               # a view that sees nothing: the background, bit for bit
            assert torch.equal(image[vv], bg.view(3, 1, 1).expand(3, S, S)) and float(alpha[vv].abs().max()) == 0.0
            assert float(depth[vv].abs().max()) == 0.0 and float(median[vv].abs().max()) == 0.0 and int(n_contrib[vv].abs().max()) == 0
        st = ref["stopped"] & ~ref["ambiguous"]
        stops += int(st.sum())
        assert bool((n_contrib[vv].long()[st] < ref["stop_pos"][st]).all())
    if R.CASES[name][0] == "stop":
        assert stops > 20, stops
    if R.CASES[name][0] == "rounds":
        assert int((a["tiles_touched"] > 256).sum()) >= 8
    if R.CASES[name][0] == "deep":
        assert max(L.numel() for L in lists) == N and int(n_contrib.max()) > min(N, 768) - 256
