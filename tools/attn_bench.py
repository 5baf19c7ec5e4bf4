#!/usr/bin/env python
"""Micro-benchmark of the attention kernels (GPU only), one shape per dispatch branch: the UNet's shapes at latent 24x40x64, the CLIP
text tower's causal call, the LGM head_dim-32 call, the CLIP image tower's head_dim-128 call and a one-wave-per-problem cross shape.
    python tools/attn_bench.py [--reps N]          us per launch (device events over N launches), TFLOP/s, served kernel"""
import argparse, ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from videomv_amd import _lib as L, ops

BRANCH = {getattr(L, "ATTN_" + n): n for n in ("SHORT", "WAVE", "Q128", "Q256", "CAUSAL", "D32", "D128")}


def bench(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fused(P, N, heads, hd, causal=False):
    """q | k | v rows (problem, token) of one buffer: self-attention of P problems of N tokens"""
    inner, BF = heads * hd, L.elem()
    qkv = torch.randn(P * N, 3 * inner, device="cuda").to(BF)
    o = torch.zeros(P * N, inner, dtype=BF, device="cuda")
    mp = lambda l: ops.seq_map(N * l, 0, l, inner=1)
    base = qkv.data_ptr()
    p = ops.attn_params(base, base + 2 * inner, base + 4 * inner, o, mp(3 * inner), mp(3 * inner), mp(3 * inner), mp(inner), P, heads, N, N,
                        hd ** -0.5, head_dim=hd, causal=causal)
    return p, (qkv, o), 4.0 * P * heads * N * N * hd * (0.5 if causal else 1.0)


def cross(P, Nq, Nk, heads, kv_div):
    """q rows (problem, token); k | v rows (kv problem, token) shared by kv_div problems (head_dim 64)"""
    inner, BF = heads * 64, L.elem()
    q = torch.randn(P * Nq, inner, device="cuda").to(BF)
    kv = torch.randn((P // kv_div) * Nk, 2 * inner, device="cuda").to(BF)
    o = torch.zeros(P * Nq, inner, dtype=BF, device="cuda")
    mp, kvm = ops.seq_map(Nq * inner, 0, inner, inner=1), ops.seq_map(Nk * 2 * inner, 0, 2 * inner, inner=1)
    p = ops.attn_params(q, kv, kv.data_ptr() + 2 * inner, o, mp, kvm, kvm, mp, P, heads, Nq, Nk, 64 ** -0.5, kv_div=kv_div)
    return p, (q, kv, o), 4.0 * P * heads * Nq * Nk * 64


def temporal(B, F, HW, heads):
    """q | k | v rows (batch, frame, pixel): one problem per (batch, pixel) over the F frames (head_dim 64)"""
    inner, BF = heads * 64, L.elem()
    qkv = torch.randn(B * F * HW, 3 * inner, device="cuda").to(BF)
    o = torch.zeros(B * F * HW, inner, dtype=BF, device="cuda")
    mp = lambda l: ops.seq_map(F * HW * l, l, HW * l, inner=HW)
    base = qkv.data_ptr()
    p = ops.attn_params(base, base + 2 * inner, base + 4 * inner, o, mp(3 * inner), mp(3 * inner), mp(3 * inner), mp(inner), B * HW, heads, F, F, 64 ** -0.5)
    return p, (qkv, o), 4.0 * B * HW * heads * F * F * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    S = ops.Stream(record=False)
    B, F = 2, 24
    shapes = [("self L0 N2560 h5", lambda: fused(B * F, 2560, 5, 64)), ("self L1 N640 h10", lambda: fused(B * F, 640, 10, 64)),
              ("self L2 N160 h20", lambda: fused(B * F, 160, 20, 64)),
              ("cross L0 N2560x77 h5", lambda: cross(B * F, 2560, 77, 5, F)), ("cross L1 N640x77 h10", lambda: cross(B * F, 640, 77, 10, F)),
              ("temporal L0 24 h5", lambda: temporal(B, F, 2560, 5)), ("temporal L1 24 h10", lambda: temporal(B, F, 640, 10)),
              # CLIP ViT-H/14 text tower (clip_text.py): 77 tokens, 16 heads of 64, causal; cond + uncond prompts
              ("clip text causal T77 h16", lambda: fused(2, 77, 16, 64, causal=True)),
              # LGM 'big' U-Net, 512-channel level (lgm.py): 4 views x 32 x 32 tokens, 16 heads of 32
              ("lgm d32 N4096 h16", lambda: fused(1, 4096, 16, 32)),
              # CLIP ViT-H/14 image tower (clip_vision.py): 257 tokens, 16 heads of 80 packed 128 wide (FLOPs counted at 128); four views
              ("clip image d128 T257 h16", lambda: fused(4, 257, 16, 128)),
              # one wave per problem with key tiles: 24 queries (a frame axis) against the 77 text tokens
              ("wave 24x77 h10", lambda: cross(B * 640, 24, 77, 10, 640))]
    for name, make in shapes:
        p, keep, fl = make()
        ms = bench(lambda: S.attention(p), args.reps)
        print(f"{name:26s} {ms * 1000:8.1f} us  {fl / ms / 1e9:7.1f} TFLOP/s  {BRANCH[L.load().vmv_attention_served_kernel(ctypes.byref(p))]}", flush=True)
        del keep


if __name__ == "__main__":
    main()
