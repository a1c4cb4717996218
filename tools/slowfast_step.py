#!/usr/bin/env python3
"""Time the `--model 2` training step (harness.slowfast_train_step) at config/slowfast.yaml size: bs 32 clips of 16 frames at 256 x 256,
UniformTemporalSubsample to 32 fast / 8 slow frames, SlowFast R50 with a 1-class head, BCE, SGD.  Prints one JSON line with ms/step,
clips/s and the step's fp32 FLOPs (convolutions and head, forward + data gradient + weight gradient; the stems take no data gradient)
as a fraction of the fp32 MFMA peak (157.3 TFLOPS).

    python tools/slowfast_step.py --steps 5 --warmup 2
    python tools/slowfast_step.py --torch-conv3d      # yardstick: the fp32 restatement of tests/slowfast_ref.py on torch's conv3d
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import harness, lib, slowfast as S  # noqa: E402

PEAK_FP32 = 157.3e12


def step_flops(B, H, W, Ts=8, Tf=32):
    """Multiply-adds x 2 of every convolution and the head for one training step (fwd, dgrad except the stems, wgrad)."""
    total = 0.0

    def conv(cin, cout, k, grid_out, stem=False):
        nonlocal total
        f = 2.0 * B * grid_out[0] * grid_out[1] * grid_out[2] * cout * cin * k[0] * k[1] * k[2]
        total += f * (2 if stem else 3)

    h, w = (H + 1) // 2, (W + 1) // 2
    conv(3, 64, (1, 7, 7), (Ts, h, w), True)
    conv(3, 8, (5, 7, 7), (Tf, h, w), True)
    h, w = (h + 1) // 2, (w + 1) // 2
    conv(8, 16, (7, 1, 1), (Ts, h, w))
    cs, cf = 80, 8
    for s in range(4):
        for i in range(S.DEPTHS[s]):
            st = S.STAGE_STRIDE[s] if i == 0 else 1
            ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
            for (cin, inner, cout, kt, T) in ((cs, S.SLOW_INNER[s], S.SLOW_OUT[s], S.SLOW_CONV_A_T[s], Ts),
                                              (cf, S.FAST_INNER[s], S.FAST_OUT[s], S.FAST_CONV_A_T[s], Tf)):
                conv(cin if i == 0 else cout, inner, (kt, 1, 1), (T, h, w))
                conv(inner, inner, (1, 3, 3), (T, ho, wo))
                conv(inner, cout, (1, 1, 1), (T, ho, wo))
                if i == 0:
                    conv(cin, cout, (1, 1, 1), (T, ho, wo))
            h, w = ho, wo
        cs, cf = S.SLOW_OUT[s], S.FAST_OUT[s]
        if s < 3:
            conv(cf, 2 * cf, (7, 1, 1), (Ts, h, w))
            cs += 2 * cf
    return total


def torch_step(model, sd, opt, videos, labels):
    from tests import slowfast_ref as R
    slow, fast = S.slowfast_input_transform(videos)
    y = R.forward(sd, slow.contiguous(), fast.contiguous(), training=True, dropout_mult=None)
    loss = F.binary_cross_entropy_with_logits(y, labels.reshape(-1, 1))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-conv3d", action="store_true", help="time the restatement on torch's own conv3d instead (yardstick)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slowfast_step.py needs a GPU")
    lib.get()
    model, opt = harness.build_slowfast(seed=0)
    g = torch.Generator().manual_seed(0)
    videos = torch.randint(0, 256, (a.batch, a.frames, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
    labels = (torch.rand(a.batch, generator=g) > 0.5).float().cuda()
    if a.torch_conv3d:
        model.blocks[6].dropout.p = 0.0
        sd = {k: v for k, v in model.state_dict(keep_vars=True).items()}
        sd["blocks.6.proj.weight"], sd["blocks.6.proj.bias"] = model.blocks[6].proj.weight, model.blocks[6].proj.bias
        opt = torch.optim.SGD(model.parameters(), lr=0.001, weight_decay=0.0001)
        step = lambda: torch_step(model, sd, opt, videos, labels)  # noqa: E731
    else:
        step = lambda: harness.slowfast_train_step(model, opt, videos, labels)  # noqa: E731
    for i in range(a.warmup):
        step()
        torch.cuda.synchronize()
        print(f"warmup step {i} done", file=sys.stderr, flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    loss = loss.item()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    fl = step_flops(a.batch, a.size, a.size)
    print(json.dumps({"workload": "slowfast_train_step" + ("_torch_conv3d" if a.torch_conv3d else ""), "batch": a.batch,
                      "frames": a.frames, "size": a.size, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 2),
                      "clips_per_s": round(1e3 * a.batch / ms, 2), "tflop_per_step": round(fl / 1e12, 3),
                      "fp32_peak_fraction": round(fl / (ms * 1e-3) / PEAK_FP32, 4), "loss": loss}))


if __name__ == "__main__":
    main()
