"""What every engine (UNet, LGM, VAE, CLIP towers) needs to record a plan of C-ABI launches: pooled activation buffers, the recording
stream with its tile-table hook, one split-K slab, and the launch forms the networks share — the implicit GEMM on packed weights, the
GroupNorm, the ResNet block, the stride-2 and nearest-x2 convolutions."""
from typing import Dict, List

import torch

from . import _lib as L
from . import ops


class Pool:
    """Size-bucketed reuse of device buffers.  All launches are stream-ordered on ONE stream, so a buffer can
    be handed to a later op as soon as its last consumer has been *recorded*."""

    def __init__(self, device):
        self.device = device
        self.free: Dict[int, List[torch.Tensor]] = {}
        self.all: List[torch.Tensor] = []
        self.bytes = 0

    def get(self, nbytes: int) -> torch.Tensor:
        nbytes = (int(nbytes) + 255) // 256 * 256
        lst = self.free.get(nbytes)
        if lst:
            return lst.pop()
        t = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.all.append(t)
        self.bytes += nbytes
        return t

    def put(self, t: torch.Tensor):
        self.free.setdefault(t.numel(), []).append(t)


class Act:
    """A [rows, C] activation living in a pooled buffer."""
    __slots__ = ("buf", "rows", "C", "dtype")

    def __init__(self, buf, rows, C, dtype=None):
        self.buf, self.rows, self.C, self.dtype = buf, rows, C, dtype or L.elem()

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def tensor(self) -> torch.Tensor:
        esz = 4 if self.dtype == torch.float32 else 2
        return self.buf[: self.rows * self.C * esz].view(self.dtype).view(self.rows, self.C)


class PlanBuilder:
    """Base of the engines.  A subclass packs its weights into ``self.wt`` (key -> device tensor) and records its plan on ``self.S``."""

    SPLITK_CAP = 8      # most K slices ops.SplitK picks for this engine's small-M GEMMs (the LGM and the VAE: 32)

    def _init_plan(self, device, taps=None, groupnorm=True, tuned=True):
        """A clean slate to record on.  taps: optional dict the engine fills with its intermediate activations (buffers are then
        never recycled).  groupnorm: the network has GroupNorms (their partial-sum workspace).  tuned: GEMMs about to be recorded take
        the measured (tile, split-K) choices of videomv_amd/tuned_gemm.json and ops.fill_rule (ops.make_tuner)."""
        self.device, self.taps = device, taps
        self.pool = Pool(device)
        self.S = ops.Stream(record=True)
        self._keep = []             # device tensors outside the pool that recorded launches point at
        self._splitk = ops.SplitK(device, cap=self.SPLITK_CAP)
        self.n_tuned, self.n_ruled, self.n_stale = 0, 0, 0      # launches forced by the table / by ops.fill_rule / table entries the library refused
        if tuned:
            self.S.tuner = ops.make_tuner(self)
        if groupnorm:
            self._gnws = torch.empty(4 << 20, dtype=torch.float32, device=device)

    def _take_weights(self, sd, packed):
        """packed: the .wt of another engine of the same kind, model and device — packed weights are immutable and shape-independent,
        so the engines of one model share ONE copy."""
        if packed is not None:
            self.wt = packed
        else:
            self.wt = {}
            self._pack(sd)

    # ------------------------------------------------------------------ buffers
    def act(self, rows, C, dtype=None) -> Act:
        esz = 4 if dtype == torch.float32 else 2
        return Act(self.pool.get(rows * C * esz), rows, C, dtype)

    def release(self, a: Act):
        if self.taps is None:
            self.pool.put(a.buf)

    rel = release

    # ------------------------------------------------------------------ launches
    def _gemm(self, label, M, segs, W, out, ldo=None, bias=None, N=None, stream=None, **kw):
        """W: key of a packed weight, a tensor, or a raw device pointer to 16-bit [N][K] rows (then N must be given; else the launch
        covers every row of W).  out: an Act, or a pointer with its row pitch ldo.  Split-K is picked here (ops.SplitK) unless the
        caller gives ksplit or the GEMM takes row statistics (a folded LayerNorm).  stream: another recorder than self.S."""
        Wt = self.wt[W] if isinstance(W, str) else W
        if N is None:
            N = Wt.shape[0]
        if "ksplit" not in kw and not kw.get("rowstat"):
            kw["ksplit"], kw["workspace"] = self._splitk.pick(M, N, segs)
        (stream or self.S).gemm(ops.gemm_params(M, N, segs, Wt, out.ptr if isinstance(out, Act) else out,
                                                ldo if ldo is not None else out.C, bias=bias, **kw), label)

    comm = None         # frame-parallel communicator (UNetEngine)

    def _gn(self, label, srcs, rows_per_stat, key, eps, silu, table: Act = None, all_frames=False) -> Act:
        """Every GroupNorm(32) (+ SiLU) of every engine: the channel concat of one or two sources, statistics per `rows_per_stat` rows,
        into a new Act — or, table given (fp32 [nstat * 2][C]), its scale / shift table for a GEMM that folds the apply pass
        (gemm_params(gn_table=...)).  The launches:
          fused          one launch where the stat group fits on chip (ops.gn_fused_cols); never to a table, never frame-parallel
          stats + second on the per-chunk partial sums: rows_per_stat = one frame.  second = apply | table
          stats + second on integer totals (all_frames: statistics over every frame; the UNet, _gn_totals): up to 256 chunks
                         per stat group, which the statistics pass folds itself.  Frame-parallel: the input is the pixel-major shard, so
                         each rank sums its HW/R pixels of all frames, the totals are all-gathered in between and every rank folds all
                         R shards in the same order (bitwise identical statistics)."""
        rows, C0 = srcs[0].rows, srcs[0].C
        C1 = srcs[1].C if len(srcs) > 1 else 0
        nstat = rows // rows_per_stat
        y = table or self.act(rows, C0 + C1)
        assert ops.gn_partial_floats(rows, rows_per_stat, C0 + C1) <= self._gnws.numel()
        params = lambda **kw: ops.gn_params(srcs[0].ptr, C0, C0, rows, rows_per_stat, self._gnws, self.wt[key + ".weight"],
                                            self.wt[key + ".bias"], eps, silu, y.ptr, C0 + C1,
                                            x1=srcs[1].ptr if C1 else None, ld1=C1, C1=C1, **kw)
        second = self.S.groupnorm_table if table else self.S.groupnorm_apply
        fused = 0 if table or (all_frames and self.comm is not None) else ops.gn_fused_cols(rows_per_stat, C0 + C1)
        if fused:
            self.S.groupnorm_fused(params(), fused, label)
        elif not all_frames:
            gnp = params()
            self.S.groupnorm_stats(gnp, label)
            second(gnp, label)
        else:
            tot, nxt, gather = self._gn_totals(nstat)
            clr = dict(totals_clear=nxt, clear_count=nstat * ops.GN_TOT)      # (second clears the NEXT norm's accumulators)
            if gather is None:
                gnp = params(totals=tot, **clr)
                self.S.groupnorm_stats(gnp, label)
                second(gnp, label)
            else:
                self.S.groupnorm_stats(params(totals=tot), label)
                second(params(totals=gather(label + ".totals.gather"), fold_ranks=self.R, **clr), label)
        return y

    def _gn_totals(self, nstat):
        """The integer-totals accumulators of the next all-frame norm (nstat stat groups) -> (its own: zero when its statistics pass
        starts, the ones its second launch clears, gather).  gather: None, or on a frame-parallel plan f(label) that records the
        all-gather of the ranks' totals -> the gathered [R] records."""
        raise NotImplementedError(f"{type(self).__name__} records no all-frame GroupNorm")

    def _conv_res(self, p, srcs, h, w, eps, skip, keys=("norm1", "norm1", "conv1", "norm2", "norm2"), conv1_kw=None, res_scale=0.0) -> Act:
        """ResNet block: GroupNorm + SiLU -> conv3x3 -> GroupNorm + SiLU -> conv3x3 + shortcut.  srcs = [x] or [x, skip] (channel
        concat, never materialised).  Where the channel count changes, the 1x1 shortcut is part of conv2's K loop (weights packed as
        `p`.conv2 = [conv2 | shortcut]; launch label `p`.conv2+`skip`); else x is conv2's residual, scaled by res_scale when given.
        keys, each below `p`: (label of norm 1, its weights, conv1's weights and label, label of norm 2, its weights).  conv1_kw: more
        arguments of conv1's launch.  The inputs are not released."""
        T, hw = srcs[0].rows, h * w
        n1, k1, c1, n2, k2 = (f"{p}.{k}" for k in keys)
        geom = ops.Geom(OH=h, OW=w, IH=h, IW=w)
        cout = self.wt[c1 + ".weight"].shape[0]
        h0 = self._gn(n1, srcs, hw, k1, eps, True)
        h1 = self.act(T, cout)
        self._gemm(p + ".conv1", T, ops.conv3x3_segs([(h0.ptr, h0.C, h0.C)]), c1 + ".weight", h1, bias=self.wt[c1 + ".bias"], geom=geom,
                   **(conv1_kw or {}))
        self.release(h0)
        h2 = self._gn(n2, [h1], hw, k2, eps, True)
        self.release(h1)
        y = self.act(T, cout)
        segs = ops.conv3x3_segs([(h2.ptr, h2.C, h2.C)])
        if sum(s.C for s in srcs) != cout:
            segs += ops.linear_segs([(s.ptr, s.C, s.C) for s in srcs])
            self._gemm(f"{p}.conv2+{skip}", T, segs, p + ".conv2.weight", y, bias=self.wt[p + ".conv2.bias"], geom=geom)
        else:
            self._gemm(p + ".conv2", T, segs, p + ".conv2.weight", y, bias=self.wt[p + ".conv2.bias"], geom=geom,
                       residual=srcs[0].ptr, ldr=srcs[0].C, res_scale=res_scale)
        self.release(h2)
        return y

    def _conv_down(self, p, x: Act, h, w, shift=0):
        """Stride-2 3x3 convolution `p` of x's images of h x w -> (y, oh, ow).  shift=1: the VAE encoder's pad-(0,1,0,1) form
        (ops.conv3x3_segs).  x is not released."""
        oh, ow = (h + 1 - shift) // 2, (w + 1 - shift) // 2
        y = self.act(x.rows // (h * w) * oh * ow, x.C)
        self._gemm(p, y.rows, ops.conv3x3_segs([(x.ptr, x.C, x.C)], shift=shift), p + ".weight", y, bias=self.wt[p + ".bias"],
                   geom=ops.Geom(OH=oh, OW=ow, IH=h, IW=w, stride=2))
        return y, oh, ow

    def _conv_up(self, p, x: Act, h, w, out=None):
        """Nearest x2 up-sampling + 3x3 convolution `p`, the up-sampling folded into the conv's gather -> (y, 2h, 2w).  x is not
        released."""
        y = out or self.act(4 * x.rows, x.C)
        self._gemm(p, y.rows, ops.conv3x3_segs([(x.ptr, x.C, x.C)]), p + ".weight", y, bias=self.wt[p + ".bias"],
                   geom=ops.Geom(OH=2 * h, OW=2 * w, IH=h, IW=w, ups=1))
        return y, 2 * h, 2 * w
