#!/usr/bin/env python3
"""Timing of the space-attention core (mt_attn_fwd / mt_attn_bwd, mode 1, plane outputs as the training step uses them) at
num-patches other than 49, with torch's fp32 scaled_dot_product_attention over the same (b, h, frame) groups as a yardstick.

    python tools/perf_attn_patches.py                                              # device-event time per call (cls + space kernels)
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/perf_attn_patches.py   # per-kernel time: OUT/**/*kernel_stats.csv

The useful work of a group is counted from its shape: 2 products of 2 n (n + 1) 64 FLOP forward (S, O), 5 backward (S again, dP, dQ,
dK, dV); the share of peak is that over the kernel's time over the fp32 MFMA peak (157.3 TFLOP/s, MI355X).  The per-call figures
printed here include the cls-query kernel (and the plane epilogue kernel backward); the per-kernel share needs the rocprofv3 run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mintime_amd  # noqa: F401
from mintime_amd import lib as L

PEAK = 157.3e12
SHAPES = [(32, 8, 8, 49), (32, 8, 8, 64), (32, 8, 16, 100)]           # (B, H, F, n); 49 is the 2 x 2-tile kernels' own figure


REPS = int(os.environ.get("PERF_REPS", "300"))     # ~0.1 s of device work per figure and more


def timeit(f, reps=None):
    reps = reps or REPS
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    lib = L.get()
    for B, H, F, n in SHAPES:
        N, inner = 1 + F * n, H * 64
        M = B * N
        g = torch.Generator(device="cuda").manual_seed(n)
        qkv = torch.randn(M, 3 * inner, device="cuda", generator=g) * 0.5
        do = torch.randn(M, inner, device="cuda", generator=g)
        mask = torch.ones(B, F, dtype=torch.uint8, device="cuda")
        ident = torch.ones(B, F, F, dtype=torch.uint8, device="cuda")
        dqkv = torch.empty(M, 3 * inner, device="cuda")
        o_p, d_p = L.planes_empty(M, inner, "cuda"), L.planes_empty(M, 3 * inner, "cuda")

        def fwd():
            L.check(lib.mt_attn_fwd(L.ptr(qkv), None, None, L.ptr(mask), L.ptr(ident), B, H, F, n, 1, 0.125, L.ptr(o_p), L.stream_ptr()), "fwd")

        def bwd():
            L.check(lib.mt_attn_bwd(L.ptr(qkv), L.ptr(do), L.ptr(dqkv), L.ptr(mask), L.ptr(ident), B, H, F, n, 1, 0.125, L.ptr(d_p),
                                    L.stream_ptr()), "bwd")

        # the same groups through torch: [B H F, 1, n + 1, 64] (cls key included), fp32
        G = B * H * F
        q = torch.randn(G, 1, n, 64, device="cuda", generator=g, requires_grad=True)
        k = torch.randn(G, 1, n + 1, 64, device="cuda", generator=g, requires_grad=True)
        v = torch.randn(G, 1, n + 1, 64, device="cuda", generator=g, requires_grad=True)
        go = torch.randn(G, 1, n, 64, device="cuda", generator=g)

        def sdpa_fwd():
            with torch.no_grad():
                torch.nn.functional.scaled_dot_product_attention(q, k, v)

        def sdpa_fwd_bwd():
            q.grad = k.grad = v.grad = None
            torch.nn.functional.scaled_dot_product_attention(q, k, v).backward(go)

        unit = 2.0 * n * (n + 1) * 64 * G
        tf, tb, sf, sfb = timeit(fwd), timeit(bwd), timeit(sdpa_fwd), timeit(sdpa_fwd_bwd)
        print(f"B {B} H {H} F {F} n {n}: {G} groups, useful GFLOP fwd {2 * unit / 1e9:.2f} bwd {5 * unit / 1e9:.2f}")
        print(f"  mt_attn_fwd (cls + space kernels)   {tf * 1e6:8.1f} us/call   {2 * unit / tf / 1e12:6.2f} TFLOP/s = {2 * unit / tf / PEAK:.3f} of the fp32 MFMA peak")
        print(f"  mt_attn_bwd (cls + space + planes)  {tb * 1e6:8.1f} us/call   {5 * unit / tb / 1e12:6.2f} TFLOP/s = {5 * unit / tb / PEAK:.3f}")
        print(f"  torch SDPA fp32 forward             {sf * 1e6:8.1f} us/call   {2 * unit / sf / 1e12:6.2f} TFLOP/s = {2 * unit / sf / PEAK:.3f}")
        print(f"  torch SDPA fp32 backward (fwd+bwd - fwd) {(sfb - sf) * 1e6:8.1f} us   {5 * unit / max(sfb - sf, 1e-9) / 1e12:6.2f} TFLOP/s = {5 * unit / max(sfb - sf, 1e-9) / PEAK:.3f}")


if __name__ == "__main__":
    main()
