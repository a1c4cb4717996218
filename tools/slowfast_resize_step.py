#!/usr/bin/env python3
"""Time the SlowFast clip ingest with ShortSideScale + CenterCropVideo (mt_sf_ingest_resize and its adjoint) with device events, one
JSON line per kernel: ms, bytes moved, TB/s.

  * the yardstick, in the same process: mt_sf_ingest on uint8 clips already at 256 x 256 (bs 32, 32 frames -> 8 slow + 32 fast);
  * mt_sf_ingest_resize on uint8 and on fp32 clips of 360 x 640 -> short side 256 (256 x 455), centre crop 256;
  * mt_sf_ingest_resize_bwd of the same geometry (its source is always fp32).

The launches alternate inside every round; a figure is the median over `--rounds` windows of `--steps` launches.  Bytes are what the
algorithm needs, from shapes: the 3 channels of every source pixel under the crop window's footprint in every distinct selected frame
(forward) or the whole fp32 clip gradient (adjoint, written), plus the packed [B][T][256][256][4] fp32 buffers of both pathways.

    python tools/slowfast_resize_step.py --rounds 5 --steps 5 --warmup 2
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import lib as L, slowfast as S  # noqa: E402


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


def footprint(n_in, n_out, first, count):
    """Source indices along one axis that the window's taps read."""
    i0, i1, _ = S.axis_taps(n_in, n_out, first, count)
    return len(set(i0.tolist()) | set(i1.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slowfast_resize_step.py needs a GPU")
    L.get()
    B, Fr, H, W, crop = a.batch, a.frames, a.height, a.width, a.crop
    gen = torch.Generator(device="cuda").manual_seed(0)
    geom = S.resize_geometry(H, W, a.side, crop) + (crop, crop)
    Hr, Wr, top, left = geom[:4]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), batch=B, frames=Fr, source=[H, W], resized=[Hr, Wr],
                          crop=[top, left, crop, crop], rounds=a.rounds, steps=a.steps, warmup=a.warmup)), flush=True)
    fi = S.frame_indices(Fr, S.NUM_FRAMES)
    si = S.frame_indices(S.NUM_FRAMES, S.NUM_FRAMES // S.ALPHA)
    sel = [fi[j] for j in si] + fi
    packed = B * len(sel) * crop * crop * 4 * 4
    pixels = footprint(H, Hr, top, crop) * footprint(W, Wr, left, crop)

    square = torch.randint(0, 256, (B, Fr, crop, crop, 3), device="cuda", generator=gen, dtype=torch.uint8)
    u8 = torch.randint(0, 256, (B, Fr, H, W, 3), device="cuda", generator=gen, dtype=torch.uint8)
    f32 = u8.float()
    d0 = torch.rand(B, len(si), crop, crop, 4, device="cuda", generator=gen)
    d1 = torch.rand(B, len(fi), crop, crop, 4, device="cuda", generator=gen)
    distinct = len(set(sel))
    runs = [
        ("mt_sf_ingest", "uint8 256x256 (yardstick)", lambda: S.ingest(square, sel, True, "bfhwc", split=len(si)),
         B * distinct * crop * crop * 3 + packed),
        ("mt_sf_ingest_resize", "uint8", lambda: S.ingest_resize(u8, sel, True, "bfhwc", geom, split=len(si)),
         B * distinct * pixels * 3 + packed),
        ("mt_sf_ingest_resize", "fp32", lambda: S.ingest_resize(f32, sel, True, "bfhwc", geom, split=len(si)),
         B * distinct * pixels * 3 * 4 + packed),
        ("mt_sf_ingest_resize_bwd", "fp32", lambda: S.ingest_resize_bwd(d0, d1, sel, tuple(f32.shape), True, "bfhwc", geom, split=len(si)),
         packed + f32.numel() * 4),
    ]
    for _, _, fn, _ in runs:
        window(fn, a.warmup)
    times = [[] for _ in runs]
    for _ in range(a.rounds):
        for t, (_, _, fn, _) in zip(times, runs):
            t.append(window(fn, a.steps))
    for t, (kernel, source, _, nbytes) in zip(times, runs):
        ms = median(t)
        print(json.dumps(dict(kernel=kernel, source=source, ms=round(ms, 3), spread_ms=[round(min(t), 3), round(max(t), 3)], bytes=nbytes,
                              TBps=round(nbytes / (ms * 1e-3) / 1e12, 3))), flush=True)


if __name__ == "__main__":
    main()
