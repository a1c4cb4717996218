#!/usr/bin/env python3
"""What the per-step metrics cost: the config-3 training step (EfficientNet-B0 + TimeSformer, B = 32 clips of 8 frames, 2
identities) timed three ways in ONE process, interleaved round by round after a warm-up of all three:

  (a) plain        harness.train_step as it is without metrics
  (b) device       harness.train_step(..., metrics=EpochMetrics): one more launch, no host read
  (c) host         the reference's way after the same step: y_pred.cpu(), a check_correct loop over the batch on the host and
                   round(loss.item(), 2) (train.py:367-374) -- one device-to-host synchronisation per step

Times are host wall clock over a window of `--steps` steps that ends in a device synchronise (a window of (c) stalls the host
every step, which device events alone would not show), median over `--rounds` windows, with min and max.
Then the two kernels alone, with device events: mt_metrics_update at B = 32 and mt_metrics_auc at n = 20 000 (a ForgeryNet-sized
validation list), and EpochMetrics.compute() at that n as host wall clock.  Prints one JSON line.

    python tools/metrics_step.py --rounds 6 --steps 10 --warmup 6
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import EpochMetrics, harness, lib, optim  # noqa: E402


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def wall(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def events(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps          # microseconds


class HostCounters:
    """check_correct (utils.py:32-57) and the running totals of train.py:369-374, on the host, as the reference keeps them."""

    def __init__(self):
        self.correct = self.positive = self.negative = self.counter = 0
        self.total_loss = 0.0

    def step(self, y_pred, labels, loss):
        y_pred = y_pred.detach().cpu()                                  # train.py:367 (the synchronisation)
        labels = labels.cpu()
        preds = [torch.sigmoid(p).numpy().round() for p in y_pred]
        for i in range(len(labels)):
            pred = int(preds[i].item())
            self.correct += int(labels[i] == pred)
            if pred == 1:
                self.positive += 1
            else:
                self.negative += 1
        self.total_loss += round(loss.item(), 2)
        self.counter += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--auc-n", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_step.py needs a GPU")
    lib.get()
    cfg, ef, tsf = harness.build_models(a.frames, seed=0, device="cuda")
    opt = harness.make_optimizer(cfg, ef, tsf)
    batch = harness.device_batch(a.batch, a.frames, 2, seed=0, device="cuda")
    m = EpochMetrics(capacity=a.batch * (a.warmup + a.rounds * a.steps + 1))
    host = HostCounters()

    def plain():
        harness.train_step(ef, tsf, opt, batch)

    def device():
        harness.train_step(ef, tsf, opt, batch, metrics=m)

    def reference():
        # train_step's body with the reference's bookkeeping behind the loss (the logits are needed on the host)
        y_pred = harness.forward(ef, tsf, batch)
        loss = optim.bce_with_logits(y_pred, batch["labels"])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        host.step(y_pred, batch["labels"], loss)

    modes = [("plain", plain), ("device", device), ("host", reference)]
    for _, fn in modes:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {name: [] for name, _ in modes}
    for r in range(a.rounds):
        order = modes[r % 3:] + modes[:r % 3]                            # rotate: no mode always runs first in a round
        for name, fn in order:
            ms[name].append(wall(fn, a.steps))
    out = {"workload": f"config 3: B={a.batch}, {a.frames} frames, 2 identities, efficientnet-b0", "rounds": a.rounds,
           "steps": a.steps, "warmup": a.warmup}
    for name, _ in modes:
        out[f"step_ms_{name}"] = round(median(ms[name]), 3)
        out[f"step_ms_{name}_min_max"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
    out["device_minus_plain_ms"] = round(median(ms["device"]) - median(ms["plain"]), 3)
    out["host_minus_plain_ms"] = round(median(ms["host"]) - median(ms["plain"]), 3)
    r = m.compute()
    assert r["n"] == a.batch * (a.warmup + a.rounds * a.steps) and not r["overflow"], r
    assert (host.correct, host.positive, host.negative) != (0, 0, 0)

    # the two kernels alone
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(a.batch, device="cuda", generator=g)
    y = (torch.rand(a.batch, device="cuda", generator=g) < 0.4).float()
    loss = torch.rand(1, device="cuda", generator=g)
    mk = EpochMetrics(capacity=a.batch)                                  # full after one update: later ones only count
    out["update_kernel_us"] = round(median([events(lambda: mk.update(x, y, loss), 200) for _ in range(5)]), 2)
    n = a.auc_n
    big = EpochMetrics(capacity=n)
    big.update(torch.randn(n, device="cuda", generator=g), (torch.rand(n, device="cuda", generator=g) < 0.4).float())
    blocks = (n + 255) // 256
    partials = torch.empty(4 * blocks, dtype=torch.int64, device="cuda")
    res = torch.empty(4, dtype=torch.int64, device="cuda")
    st = lib.stream_ptr()

    def auc():
        lib.check(lib.get().mt_metrics_auc(lib.ptr(big.store_scores), lib.ptr(big.store_labels), n, lib.ptr(partials), lib.ptr(res), st),
                  "mt_metrics_auc")
    events(auc, 10)
    out["auc_n"] = n
    out["auc_kernels_us"] = round(median([events(auc, 20) for _ in range(5)]), 1)
    big.compute()
    out["compute_wall_ms"] = round(median([wall(big.compute, 3) for _ in range(5)]), 3)
    out["auc"] = round(big.compute()["auc"], 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
