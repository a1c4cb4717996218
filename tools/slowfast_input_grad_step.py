#!/usr/bin/env python3
"""Time SlowFast's input-clip gradient at config/slowfast.yaml size (bs 32, 256 x 256, 32 frames -> 8 slow + 32 fast) with device
events, one JSON line per figure:

  * mt_sf_stem_dgrad on the slow and the fast stem, per launch, next to the yardstick of the same run: mt_conv3d_wgrad on the same
    two stems (the same tensors and exactly the same multiply-add count as the data gradients).  The four launches alternate inside
    every round; the figure is the median over `--rounds` windows of `--steps` launches.
    Criterion: the two data-gradient launches together take no longer than the two weight-gradient launches together.
  * mt_sf_ingest_bwd (both pathways -> the fp32 clip batch), per launch;
  * harness.slowfast_input_gradient in eval mode with every parameter frozen (the saliency setting), the eval forward and the training
    step, per call.

Bounds: bytes = dz read + dx written over 4.2 TB/s (the read-mostly stream rate DESIGN.md section 3 gives for this GPU), multiply-adds
x 2 of the useful taps over the fp32 MFMA peak (157.3 TFLOPS).

    python tools/slowfast_input_grad_step.py --rounds 5 --steps 5 --warmup 2
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import harness, lib as L, slowfast as S, slowfast_engine as E  # noqa: E402

PEAK_FP32 = 157.3e12
HBM_STREAM = 4.2e12


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


def stem_launches(B, T, H, W, kt, K, gen):
    """(dgrad launch, wgrad launch, bytes, flops) of one stem on random operands."""
    lib = L.get()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = E.Fm(torch.randn(B * T * H * W, 4, device="cuda", generator=gen), B, T, H, W)
    x.t[:, 3] = 0
    dz = E.Fm(torch.randn(B * T * Ho * Wo, K, device="cuda", generator=gen), B, T, Ho, Wo)
    w = torch.randn(K, 3, kt, 7, 7, device="cuda", generator=gen) / (3 * kt * 49) ** 0.5
    wt = E._pack_w_stem_dgrad(w)
    dx = torch.empty(B, T, H, W, 4, device="cuda")
    conv = E.Conv("w", (kt, 7, 7), (1, 2, 2), (kt // 2, 3, 3))
    d, _ = E._desc(x, conv.k, conv.s, conv.p, K, dz.ld)
    splits = int(lib.mt_conv3d_wgrad_splits(C.byref(d)))
    kd = kt * 49 * 4
    dwp = torch.empty(K, kd, device="cuda")
    ws = torch.empty(splits * K * kd, device="cuda") if splits > 1 else None
    st = L.stream_ptr()

    def dgrad():
        L.check(lib.mt_sf_stem_dgrad(L.ptr(dz.t), dz.ld, L.ptr(wt), L.ptr(dx), B, T, H, W, kt, K, st), "mt_sf_stem_dgrad")

    def wgrad():
        L.check(lib.mt_conv3d_wgrad(C.byref(d), L.ptr(x.t), None, None, L.ptr(dz.t), L.ptr(dwp), L.ptr(ws), splits, st), "mt_conv3d_wgrad")

    nbytes = dz.t.numel() * 4 + dx.numel() * 4
    flops = 2.0 * B * T * Ho * Wo * K * kt * 49 * 3
    return dgrad, wgrad, nbytes, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slowfast_input_grad_step.py needs a GPU")
    L.get()
    B, H = a.batch, a.size
    gen = torch.Generator(device="cuda").manual_seed(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), batch=B, frames=a.frames, size=H, rounds=a.rounds, steps=a.steps,
                          warmup=a.warmup)), flush=True)

    # 1. the stems' data gradients against the weight gradients of the same stems, alternating
    names = ("dgrad_slow", "wgrad_slow", "dgrad_fast", "wgrad_fast")
    ds, ws_, bs, fs = stem_launches(B, S.NUM_FRAMES // S.ALPHA, H, H, 1, 64, gen)
    df, wf, bf, ff = stem_launches(B, S.NUM_FRAMES, H, H, 5, 8, gen)
    fns = (ds, ws_, df, wf)
    for fn in fns:
        window(fn, a.warmup)
    times = {n: [] for n in names}
    for _ in range(a.rounds):
        for n, fn in zip(names, fns):
            times[n].append(window(fn, a.steps))
    ms = {n: median(v) for n, v in times.items()}
    for n, nbytes, flops in (("dgrad_slow", bs, fs), ("dgrad_fast", bf, ff)):
        t = ms[n] * 1e-3
        print(json.dumps(dict(kernel="mt_sf_stem_dgrad", stem=n[6:], ms=round(ms[n], 3), spread_ms=[round(min(times[n]), 3), round(max(times[n]), 3)],
                              bytes=nbytes, TBps=round(nbytes / t / 1e12, 3), byte_bound_fraction=round(nbytes / HBM_STREAM / t, 3),
                              gflop=round(flops / 1e9, 1), TFLOPS=round(flops / t / 1e12, 1), mfma_bound_fraction=round(flops / PEAK_FP32 / t, 3))),
              flush=True)
    for n in ("wgrad_slow", "wgrad_fast"):
        print(json.dumps(dict(kernel="mt_conv3d_wgrad", stem=n[6:], ms=round(ms[n], 3),
                              spread_ms=[round(min(times[n]), 3), round(max(times[n]), 3)])), flush=True)
    dsum, wsum = ms["dgrad_slow"] + ms["dgrad_fast"], ms["wgrad_slow"] + ms["wgrad_fast"]
    print(json.dumps(dict(criterion="both mt_sf_stem_dgrad launches <= both stem mt_conv3d_wgrad launches", dgrad_ms=round(dsum, 3),
                          wgrad_ms=round(wsum, 3), met=bool(dsum <= wsum))), flush=True)
    del ds, ws_, df, wf, fns
    torch.cuda.empty_cache()

    # 2. the ingest's adjoint
    videos = torch.randint(0, 256, (B, a.frames, H, H, 3), device="cuda", generator=gen, dtype=torch.uint8).float()
    fi = S.frame_indices(a.frames, S.NUM_FRAMES)
    si = S.frame_indices(S.NUM_FRAMES, S.NUM_FRAMES // S.ALPHA)
    sel = [fi[j] for j in si] + fi
    d0 = torch.randn(B, len(si), H, H, 4, device="cuda", generator=gen)
    d1 = torch.randn(B, len(fi), H, H, 4, device="cuda", generator=gen)

    def adjoint():
        S.ingest_bwd(d0, d1, sel, tuple(videos.shape), True, "bfhwc", split=len(si))
    window(adjoint, a.warmup)
    t = median([window(adjoint, a.steps) for _ in range(a.rounds)])
    nbytes = (d0.numel() + d1.numel()) * 4 + videos.numel() * 4
    print(json.dumps(dict(kernel="mt_sf_ingest_bwd", ms=round(t, 3), bytes=nbytes, TBps=round(nbytes / (t * 1e-3) / 1e12, 3))), flush=True)
    del d0, d1
    torch.cuda.empty_cache()

    # 3. whole passes
    model, opt = harness.build_slowfast(seed=0)
    labels = (torch.rand(B, device="cuda", generator=gen) > 0.5).float()

    def timed(name, fn):
        window(fn, a.warmup)
        v = [window(fn, a.steps) for _ in range(a.rounds)]
        print(json.dumps(dict(workload=name, ms=round(median(v), 2), spread_ms=[round(min(v), 2), round(max(v), 2)])), flush=True)

    timed("slowfast_train_step", lambda: harness.slowfast_train_step(model, opt, videos, labels))
    model.eval()
    timed("slowfast_eval_step", lambda: harness.slowfast_eval_step(model, videos))
    for p in model.parameters():
        p.requires_grad_(False)
    timed("slowfast_input_gradient (eval, frozen)", lambda: harness.slowfast_input_gradient(model, videos, labels))


if __name__ == "__main__":
    main()
