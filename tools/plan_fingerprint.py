#!/usr/bin/env python
"""Fingerprints of the recorded launch plans (no GPU): every engine of a fixed matrix is built on torch.device("cpu") with zero weights,
its launches are recorded (not run) with the real library loaded for its host-side answers (vmv_gemm_*_ok / pick_tile / validate), and
each recorded op of `S` (and `Sctx`) becomes one line: stream, op code, label and every field of the ctypes parameter block, nested
structs and arrays included.  Pointers are made address-independent: null -> 0, a pointer into the i-th buffer of `eng.pool.all` ->
("pool", i, offset), anything else -> ("ext", k) with k the order of first appearance of that exact value.  The fingerprint of an
engine is its op count, a count per op code and the sha256 of those lines: two trees that give the same fingerprints record the same
launches in the same order with the same parameters and the same buffer reuse.

  python tools/plan_fingerprint.py [--root TREE] [--only NAME ...] [--out FILE.json] [--dump DIR]

--root: the tree whose `videomv_amd` is fingerprinted (default: this one; it needs its built videomv_amd/lib).  Only public
constructors are used, so an older checkout works.  --out merges the result into FILE.json under the element type in use
("fp16" | "bf16", VMV_DTYPE); --dump writes the full line listing of every engine to DIR/<name>.txt (diff two dumps to find the first
differing op).  tests/test_plan_fingerprint_cpu.py compares this tree with tests/golden/plan_fingerprints.json."""
import argparse
import bisect
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

FULL = dict(in_dim=4, dim=320, context_dim=1024, out_dim=4, dim_mult=[1, 2, 4, 4], num_heads=8, head_dim=64, num_res_blocks=2,
            attn_scales=[1.0, 0.5, 0.25], camera_dim=16, use_camera_condition=True, use_fps_condition=False)
TINY = dict(in_dim=4, dim=64, context_dim=1024, out_dim=4, dim_mult=[1, 2], num_heads=2, head_dim=64, num_res_blocks=1,
            attn_scales=[1.0, 0.5], camera_dim=16, use_camera_condition=True, use_fps_condition=False)
VAE_DD = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)


# ------------------------------------------------------------------------------------------------- recording without a device
@contextlib.contextmanager
def recording_only():
    """ops.Stream records its launches into Python lists only (no C plan, nothing is launched): what tests/plan_interp.install does to
    the recorder, without the interpreter."""
    from videomv_amd import _lib as L, ops
    saved = ops.Stream.__init__, ops.Stream._go

    def init(self, record=False):
        self.lib = L.load()      # symbols only
        self.record, self.plan = record, None
        self.keep, self.nops, self.labels, self.recorded, self.graph = [], 0, [], [], None

    def go(self, op, params, fn, label):
        if not self.record:
            raise RuntimeError(f"eager launch {label!r} while fingerprinting")
        self.labels.append(label)
        self.recorded.append((op, params))
        self.nops += 1

    ops.Stream.__init__, ops.Stream._go = init, go
    try:
        yield
    finally:
        ops.Stream.__init__, ops.Stream._go = saved


@contextlib.contextmanager
def environment(**env):
    """The VMV_* switches of one case: every other VMV_* variable is removed for its duration (the element type stays), and the cached
    tile table is read again under them."""
    from videomv_amd import ops
    saved, table = dict(os.environ), ops._TUNED
    for k in list(os.environ):
        if k.startswith("VMV_") and k not in ("VMV_DTYPE", "VMV_LIB_DIR"):
            del os.environ[k]
    os.environ.update(env)
    ops._TUNED = None
    try:
        yield
    finally:
        os.environ.clear()
        os.environ.update(saved)
        ops._TUNED = table


# ------------------------------------------------------------------------------------------------- lines
class _Pointers:
    def __init__(self, pool):
        bufs = sorted((t.data_ptr(), t.numel(), i) for i, t in enumerate(pool.all))
        self.starts, self.bufs, self.ext = [b[0] for b in bufs], bufs, {}

    def name(self, v):
        if not v:
            return 0
        j = bisect.bisect_right(self.starts, v) - 1
        if j >= 0 and v < self.bufs[j][0] + self.bufs[j][1]:
            return ("pool", self.bufs[j][2], v - self.bufs[j][0])
        return ("ext", self.ext.setdefault(v, len(self.ext)))


def _fields(obj, ptrs):
    out = []
    for name, typ in obj._fields_:
        v = getattr(obj, name)
        if typ is C.c_void_p:
            out.append((name, ptrs.name(v)))
        elif isinstance(v, C.Structure):
            out.append((name, _fields(v, ptrs)))
        elif isinstance(v, C.Array):
            out.append((name, [_fields(e, ptrs) if isinstance(e, C.Structure) else e for e in v]))
        else:
            out.append((name, v))
    return out


def plan_lines(eng):
    ptrs = _Pointers(eng.pool)
    lines = []
    for sname in ("S", "Sctx"):
        S = getattr(eng, sname, None)
        if S is None:
            continue
        for (op, p), label in zip(S.recorded, S.labels):
            lines.append(repr((sname, int(op), label, _fields(p, ptrs))))
    return lines


def fingerprint(eng, dump=None):
    lines = plan_lines(eng)
    if dump:
        with open(dump, "w") as f:
            f.write("\n".join(lines) + "\n")
    ops, by_op = {}, {}
    for ln in lines:
        sname, code = ln[1:].split(", ")[:2]
        ops[sname.strip("'")] = ops.get(sname.strip("'"), 0) + 1
        by_op[code] = by_op.get(code, 0) + 1
    return dict(ops=ops, by_op=dict(sorted(by_op.items(), key=lambda kv: int(kv[0]))),
                sha256=hashlib.sha256("\n".join(lines).encode()).hexdigest())


# ------------------------------------------------------------------------------------------------- the matrix
def _zeros(shapes):
    import torch
    return {k: torch.zeros(s) for k, s in shapes.items()}


def _unet_full(emit):
    import torch
    from videomv_amd.comm import SimComm
    from videomv_amd.unet_engine import UNetEngine, param_shapes
    dev = torch.device("cpu")
    sd = _zeros(param_shapes(FULL))
    with environment():
        e64 = UNetEngine(FULL, sd, 2, 24, 40, 64, 77, dev, n_t=1, share_prefix=True)
        emit("unet.full.B2.24x40x64.shared", e64)
        packed = e64.packed
        del e64
        emit("unet.full.B2.24x32x32.shared", UNetEngine(FULL, sd, 2, 24, 32, 32, 77, dev, n_t=1, share_prefix=True, packed=packed))
        emit("unet.full.B2.24x40x64.sim8", UNetEngine(FULL, sd, 2, 24, 40, 64, 77, dev, n_t=1, comm=SimComm(8, 0), packed=packed))
        emit("unet.full.B4.24x32x32.shared", UNetEngine(FULL, sd, 4, 24, 32, 32, 77, dev, n_t=1, share_prefix=True, packed=packed))
    with environment(VMV_FP_TEMPORAL="kv_gather"):
        emit("unet.full.B1.24x40x64.sim8.kv_gather", UNetEngine(FULL, sd, 1, 24, 40, 64, 77, dev, n_t=1, comm=SimComm(8, 0), packed=packed))
    with environment(VMV_FF_FUSED="1"):
        emit("unet.full.B2.24x40x64.shared.ff_fused", UNetEngine(FULL, sd, 2, 24, 40, 64, 77, dev, n_t=1, share_prefix=True, packed=packed))
    del packed, sd
    # UNetSD_I2VGen's trunk (unet_i2vgen.py: in_dim + concat_dim input channels, 77 text + 64 local-image + 4 CLIP-image tokens)
    arch = dict(FULL, in_dim=8)
    with environment():
        emit("unet.i2vgen.B2.24x32x32.shared", UNetEngine(arch, _zeros(param_shapes(arch)), 2, 24, 32, 32, 145, dev, n_t=1, share_prefix=True))


def _unet_tiny(emit):
    import torch
    from videomv_amd.unet_engine import UNetEngine, param_shapes
    dev = torch.device("cpu")
    sd = _zeros(param_shapes(TINY))
    mk = lambda cfg=TINY, w=sd, **kw: UNetEngine(cfg, w, 2, 3, 8, 8, 5, dev, n_t=2, **kw)
    with environment():
        emit("unet.tiny", mk())
        emit("unet.tiny.taps", mk(taps={}))
        fps = dict(TINY, use_fps_condition=True)
        emit("unet.tiny.fps", mk(fps, _zeros(param_shapes(fps))))
        eng = mk()
        eng._rerecord()
        emit("unet.tiny.rerecord", eng)
        emit("unet.tiny.shared", UNetEngine(TINY, sd, 2, 3, 8, 8, 5, dev, n_t=1, share_prefix=True))
    for name, env in (("fold_ln0", dict(VMV_FOLD_LN="0")), ("ln_inline", dict(VMV_LN_INLINE="1")), ("tqa0", dict(VMV_TQA="0")),
                      ("gn_fused0", dict(VMV_GN_FUSED="0"))):
        with environment(**env):
            emit("unet.tiny." + name, mk())
    # one K = 320 level (the head-major q | k | v copies are packed) with the fused temporal attention switched off
    one = dict(TINY, dim=320, dim_mult=[1], num_heads=5, attn_scales=[1.0])
    with environment(VMV_TQA="0"):
        emit("unet.dim320.tqa0", UNetEngine(one, _zeros(param_shapes(one)), 2, 6, 4, 4, 5, dev, n_t=2))


def _lgm(emit):
    import torch
    from videomv_amd.lgm import LgmEngine, LgmOptions, lgm_param_shapes
    dev, opt = torch.device("cpu"), LgmOptions()
    sd = _zeros(lgm_param_shapes(opt))
    with environment():
        one = LgmEngine(opt, sd, opt.input_size, opt.input_size, dev)
        emit("lgm.big.256.batch1", one)
        emit("lgm.big.256.batch2", LgmEngine(opt, sd, opt.input_size, opt.input_size, dev, batch=2, packed=one.wt))
        emit("lgm.big.256.taps", LgmEngine(opt, sd, opt.input_size, opt.input_size, dev, taps={}, packed=one.wt))
        # head_dim 16: the GEMM-built attention (neither flash head size)
        small = LgmOptions(down_channels=(64, 128, 256), down_attention=(False, False, True), up_channels=(256, 128), up_attention=(True, False),
                           input_size=32, splat_size=32, output_size=64)
        emit("lgm.small.32", LgmEngine(small, _zeros(lgm_param_shapes(small)), 32, 32, dev))


def _vae(emit):
    import torch
    from videomv_amd.autoencoder import VaeDecoderEngine, VaeEncoderEngine, vae_param_shapes
    dev = torch.device("cpu")
    sd = _zeros(vae_param_shapes(VAE_DD, 4))
    with environment():
        dec = VaeDecoderEngine(VAE_DD, sd, 8, 40, 64, dev)
        emit("vae.decoder.n8.40x64", dec)
        emit("vae.encoder.n4.256x256", VaeEncoderEngine(VAE_DD, sd, 4, 256, 256, dev))
    with environment(VMV_VAE_ATTN_BATCHED="0"):
        emit("vae.decoder.n8.40x64.attn_per_frame", VaeDecoderEngine(VAE_DD, sd, 8, 40, 64, dev, packed=dec.wt))


def _clip(emit):
    import torch
    from videomv_amd.clip_text import ClipTextEngine, ClipTextOptions, clip_text_shapes
    from videomv_amd.clip_vision import ClipVisionEngine, ClipVisionOptions, clip_vision_shapes
    dev = torch.device("cpu")
    with environment():
        to = ClipTextOptions()
        sd = _zeros(clip_text_shapes(to))
        t1 = ClipTextEngine(to, sd, 1, dev)
        emit("clip.text.B1", t1)
        emit("clip.text.B2.donor", ClipTextEngine(to, sd, 2, dev, donor=t1))
        emit("clip.text.B1.taps", ClipTextEngine(to, sd, 1, dev, taps={}, donor=t1))
        del t1, sd
        vo = ClipVisionOptions()
        emit("clip.vision.B1", ClipVisionEngine(vo, _zeros(clip_vision_shapes(vo)), 1, dev))


GROUPS = dict(unet_full=_unet_full, unet_tiny=_unet_tiny, lgm=_lgm, vae=_vae, clip=_clip)


def fingerprints(only=None, dump=None, log=None):
    """{engine name: fingerprint} of the matrix (`only`: group names, default all)."""
    out = {}

    def emit(name, eng):
        out[name] = fingerprint(eng, os.path.join(dump, name + ".txt") if dump else None)
        if log:
            log(f"{name}: ops {out[name]['ops']}  {out[name]['sha256'][:16]}")

    if dump:
        os.makedirs(dump, exist_ok=True)
    with recording_only():
        for g in (only or list(GROUPS)):
            GROUPS[g](emit)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", nargs="*", choices=list(GROUPS))
    ap.add_argument("--out")
    ap.add_argument("--dump")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from videomv_amd import _lib as L
    fp = fingerprints(a.only, a.dump, log=lambda s: print(s, flush=True))
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc.setdefault(L.elem_name(), {}).update(fp)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
