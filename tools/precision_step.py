#!/usr/bin/env python3
"""Time the matmul precision tiers against each other: the config-3 training step (EfficientNet-B0 + TimeSformer, B = 32 clips of
8 frames, 2 identities) and its eval forward, at "highest" (six piece products) and "high" (three) in the SAME process, interleaved
round by round after a warm-up at both tiers.  The tier is read at dispatch, so the same models and the same recorded launch plans
serve both.  Prints one JSON line with ms/step for both tiers and the ratio high / highest.

    python tools/precision_step.py --rounds 6 --steps 5 --warmup 6
    python tools/precision_step.py --config 5                # Xception "XS": B = 32 x 16 frames x 3 identities
    python tools/precision_step.py --only high --leg train_step --rounds 1    # one tier, one leg (a profiler run of the high step)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import harness, lib  # noqa: E402

CONFIGS = {3: dict(B=32, frames=8, ids=2, xs=False), 5: dict(B=32, frames=16, ids=3, xs=True)}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=6, help="interleaved rounds; each times `steps` steps per tier and leg")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6, help="untimed steps per tier and leg before the first round")
    ap.add_argument("--only", choices=["highest", "high"], default=None)
    ap.add_argument("--leg", choices=["train_step", "eval_forward"], default=None, help="one leg only (a profiler run of the step)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("precision_step.py needs a GPU")
    lib.get()
    wl = CONFIGS[a.config]
    B = a.batch or wl["B"]
    build = harness.build_models_xs if wl["xs"] else harness.build_models
    cfg, ef, tsf = build(wl["frames"], seed=0, device="cuda")
    opt = harness.make_optimizer(cfg, ef, tsf)
    batch = harness.device_batch(B, wl["frames"], wl["ids"], seed=0, device="cuda")
    tiers = [a.only] if a.only else ["highest", "high"]

    def train():
        return harness.train_step(ef, tsf, opt, batch)

    def evaluate():
        ef.eval(), tsf.eval()
        harness.eval_step(ef, tsf, batch)
        ef.train(), tsf.train()

    legs = {"train_step": train, "eval_forward": evaluate}
    if a.leg:
        legs = {a.leg: legs[a.leg]}
    start = lib.get_matmul_precision()
    ms = {leg: {t: [] for t in tiers} for leg in legs}
    try:
        for t in tiers:
            lib.set_matmul_precision(t)
            for leg, fn in legs.items():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            print(f"warm-up at {t} done", file=sys.stderr, flush=True)
        for r in range(a.rounds):
            for t in (tiers if r % 2 == 0 else tiers[::-1]):          # alternate the order: neither tier always runs on the warmer chip
                lib.set_matmul_precision(t)
                for leg, fn in legs.items():
                    ms[leg][t].append(timed(fn, a.steps))
        lib.set_matmul_precision(tiers[-1])
        loss = float(train().item())
    finally:
        lib.set_matmul_precision(start)
    out = {"workload": f"config {a.config}: B={B}, {wl['frames']} frames, {wl['ids']} identities, "
                       f"{'xception' if wl['xs'] else 'efficientnet-b0'}", "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup}
    for leg in legs:
        for t in tiers:
            out[f"{leg}_ms_{t}"] = round(median(ms[leg][t]), 3)
            out[f"{leg}_ms_{t}_min_max"] = [round(min(ms[leg][t]), 3), round(max(ms[leg][t]), 3)]
        if len(tiers) == 2:
            out[f"{leg}_ratio_high_over_highest"] = round(median(ms[leg]["high"]) / median(ms[leg]["highest"]), 4)
    out["last_loss_at_" + tiers[-1]] = round(loss, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
