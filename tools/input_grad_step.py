#!/usr/bin/env python3
"""Time the stem data-gradient kernel (csrc/stem_dgrad.hip) alone with device events: mt_stem_conv_dgrad at 256 crops of 224^2
(EfficientNet-B0's stem, TF-SAME) and mt_stem_conv_dgrad_valid at 512 crops of 299^2 (Xception's conv1).  Prints one JSON line per
shape: microseconds per launch (median of `--rounds` windows of `--steps` launches), the algorithmic bytes
(N*Ho*Wo*32*4*2 read + N*H*W*3*4 written) and the byte rate.

    python tools/input_grad_step.py --rounds 7 --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import lib as L  # noqa: E402

SHAPES = [("effnet_stem_same", 256, 224, False), ("xception_conv1_valid", 512, 299, True)]


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_step.py needs a GPU")
    lib = L.get()
    for name, N, H, valid in SHAPES:
        Ho = (H - 3) // 2 + 1 if valid else (H + 1) // 2
        g = torch.Generator(device="cuda").manual_seed(0)
        du = torch.randn(N * Ho * Ho, 32, device="cuda", generator=g)
        z = torch.randn(N * Ho * Ho, 32, device="cuda", generator=g)
        kabc = torch.rand(3, 32, device="cuda", generator=g) + 0.5
        w = torch.randn(32, 3, 3, 3, device="cuda", generator=g)
        dx = torch.empty(N, H, H, 3, device="cuda")
        fn = lib.mt_stem_conv_dgrad_valid if valid else lib.mt_stem_conv_dgrad
        st = L.stream_ptr()

        def launch():
            L.check(fn(L.ptr(du), L.ptr(z), L.ptr(kabc), L.ptr(w), L.ptr(dx), N, H, H, st), name)
        window(launch, a.warmup)
        ms = median([window(launch, a.steps) for _ in range(a.rounds)])
        nbytes = N * Ho * Ho * 32 * 4 * 2 + N * H * H * 3 * 4
        print(json.dumps(dict(kernel=name, N=N, H=H, W=H, us=round(ms * 1e3, 1), bytes=nbytes, TBps=round(nbytes / (ms * 1e-3) / 1e12, 3))))
        del du, z, dx


if __name__ == "__main__":
    main()
