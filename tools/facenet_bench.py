#!/usr/bin/env python3
"""What the FaceNet InceptionResnetV1 embedder costs on the device (mintime_amd.facenet, csrc/facenet.hip), timed with device
events, warm, as the median (with min and max) of `--rounds` windows of back-to-back calls:

  (a) `embed_crops` of T = 200 and T = 800 uint8 faces at 128 x 128: ms, faces/s, and the fp32 MFMA rate 2 x 811.4 M x T FLOP over
      the call time as a fraction of the 157.3 TFLOP/s peak (a whole-call rate: launches and the non-convolution kernels included);
  (b) the five heaviest layer shapes of that network (by multiply-adds per launch times launches per forward, T = 200), `mt_conv2d_fwd` with bias + ReLU in its
      epilogue against `mt_conv3d_fwd` run as a 2-D convolution (T = 1, kt = 1) followed by a separate bias + ReLU pass
      (`mt_sf_bn_relu_fwd` with scale 1).  The two variants alternate window by window in this process and their outputs are
      compared; `spread` is (max - min) / median of a variant's own windows;
  (c) every launch of the T = 200 launch list timed alone and summed per stage of the network;
  (d) the plain-torch restatement (tests/facenet_ref.py) on the device, i.e. MIOpen -- an outside second opinion only.

Prints a text report (profiles/facenet_embed.txt is one run of it).

    python tools/facenet_bench.py --rounds 7
"""
import argparse
import ctypes as C
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "2")        # MIOpen's fast find: the second opinion should not spend minutes searching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402
from mintime_amd import facenet_engine as E  # noqa: E402
from mintime_amd import lib as L  # noqa: E402
from tests import facenet_ref as R  # noqa: E402

PEAK_TFLOPS = 157.3
MAC_PER_FACE_128 = 811.4e6


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls                # milliseconds per call


def stats(v):
    m = median(v)
    return {"median": m, "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / m}


def alternate(fns, rounds, calls):
    """fns: {name: fn}; every round times each variant once, in turn."""
    for fn in fns.values():
        window(fn, max(3, calls // 4))                # warm: code objects loaded, clocks up
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, calls))
    return {k: stats(v) for k, v in out.items()}


def fmt(s, unit="ms"):
    return f"{s['median']:9.4f} {unit} (min {s['min']:.4f}, max {s['max']:.4f}, spread {100 * s['spread']:.1f} %)"


def whole_network(model, T, rounds):
    crops = torch.randint(0, 256, (T, 128, 128, 3), generator=torch.Generator().manual_seed(T), dtype=torch.uint8).cuda()
    s = alternate({"embed": lambda: model.embed_crops(crops)}, rounds, 5)["embed"]
    tf = 2 * MAC_PER_FACE_128 * T / (s["median"] * 1e-3) / 1e12
    print(f"embed_crops T = {T:4d} at 128 x 128: {fmt(s)}  {T / (s['median'] * 1e-3):9.0f} faces/s  "
          f"{tf:6.2f} TFLOP/s = {100 * tf / PEAK_TFLOPS:.1f} % of the fp32 MFMA peak (whole call)")
    return crops


def heaviest_layers(model, T, count=5):
    b = E._Builder(model.engine(), T, 128, 128)
    E._program(b, model)
    seen = {}
    for op in b.ops:
        if op[0] != "conv":
            continue
        d = op[1]
        key = (d.H, d.W, d.C, d.K, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw)
        macs = d.N * d.Ho * d.Wo * d.K * d.kh * d.kw * d.C
        seen[key] = (macs, seen.get(key, (0, 0))[1] + 1)
    return sorted(seen.items(), key=lambda kv: -kv[1][0] * kv[1][1])[:count]


def layer(key, macs, uses, T, rounds):
    H, W, Cc, K, kh, kw, sh, sw, ph, pw = key
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    g = torch.Generator().manual_seed(K + Cc)
    x = torch.randn(T * H * W, Cc, generator=g).cuda()
    w = (torch.randn(K, kh, kw, Cc, generator=g) * (2.0 / (kh * kw * Cc)) ** 0.5).cuda()
    bias = torch.randn(K, generator=g).cuda()
    ones = torch.ones(K, device="cuda")
    y2, z3, y3 = (torch.empty(T * Ho * Wo, K, device="cuda") for _ in range(3))
    d2 = L.Conv2dDesc()
    d2.N, d2.H, d2.W, d2.C, d2.Ho, d2.Wo, d2.K = T, H, W, Cc, Ho, Wo, K
    d2.kh, d2.kw, d2.sh, d2.sw, d2.ph, d2.pw, d2.act, d2.res_scale = kh, kw, sh, sw, ph, pw, 1, 1.0
    d2.ldx, d2.ldy, d2.ldr = Cc, K, 0
    d3 = L.Conv3dDesc()
    d3.N, d3.T, d3.H, d3.W, d3.C, d3.To, d3.Ho, d3.Wo, d3.K = T, 1, H, W, Cc, 1, Ho, Wo, K
    d3.kt, d3.kh, d3.kw, d3.st, d3.sh, d3.sw, d3.pt, d3.ph, d3.pw = 1, kh, kw, 1, sh, sw, 0, ph, pw
    d3.ldx, d3.ldy = Cc, K
    lib, st = L.get(), L.stream_ptr()
    rows = T * Ho * Wo

    def new():
        L.check(lib.mt_conv2d_fwd(C.byref(d2), L.ptr(x), L.ptr(w), L.ptr(bias), None, L.ptr(y2), st), "mt_conv2d_fwd")

    def old():
        L.check(lib.mt_conv3d_fwd(C.byref(d3), L.ptr(x), None, None, L.ptr(w), L.ptr(z3), 0, None, None, st), "mt_conv3d_fwd")
        L.check(lib.mt_sf_bn_relu_fwd(L.ptr(z3), K, L.ptr(ones), L.ptr(bias), None, 0, None, None, L.ptr(y3), K, rows, K, st),
                "mt_sf_bn_relu_fwd")

    calls = max(5, min(200, int(2e10 / macs)))
    r = alternate({"conv2d": new, "conv3d+pass": old}, rounds, calls)
    diff = (y2 - y3).abs().max().item()
    tf = 2 * macs / (r["conv2d"]["median"] * 1e-3) / 1e12
    ratio = r["conv2d"]["median"] / r["conv3d+pass"]["median"]
    print(f"{H}x{W} C={Cc} -> K={K} k=({kh},{kw}) s=({sh},{sw}) p=({ph},{pw}), {rows} rows, {macs / 1e9:.2f} GMAC, used {uses}x")
    print(f"    mt_conv2d_fwd (bias + ReLU fused)   {fmt(r['conv2d'])}  {tf:6.2f} TFLOP/s = {100 * tf / PEAK_TFLOPS:.1f} % of peak")
    print(f"    mt_conv3d_fwd + bias/ReLU pass      {fmt(r['conv3d+pass'])}")
    print(f"    new / old = {ratio:.3f}; max |difference of the outputs| = {diff:.3e}")
    return ratio, max(r["conv2d"]["spread"], r["conv3d+pass"]["spread"])


STAGES = (("stem: conv2d_1a .. conv2d_4b + maxpool_3a", 7), ("repeat_1: 5 x Block35", 30), ("mixed_6a", 5), ("repeat_2: 10 x Block17", 40),
          ("mixed_7a", 6), ("repeat_3 + block8: 6 x Block8", 24), ("avgpool_1a + last_linear/last_bn", 2))


def stages(model, T, rounds):
    """Every launch of the T-face launch list timed on its own (windows of 20 back-to-back repeats; a launch reads and writes different
    buffers, so repeating it changes nothing), summed per stage.  Launches run back to back here, so the sums leave out the gaps between
    dependent launches of a real call."""
    eng = model.engine()
    prog = eng.program(torch.device("cuda", torch.cuda.current_device()), T, 128, 128)
    b = E._Builder(eng, T, 128, 128)
    E._program(b, model)
    st = L.stream_ptr()
    assert len(prog["calls"]) == len(b.ops) == sum(n for _, n in STAGES)
    times, macs = [], []
    for (fn, args), op in zip(prog["calls"], b.ops):
        times.append(alternate({"x": lambda: fn(*args, st)}, max(3, rounds // 2), 20)["x"]["median"])
        d = op[1] if op[0] == "conv" else None
        macs.append(d.N * d.Ho * d.Wo * d.K * d.kh * d.kw * d.C if d is not None else 0)
    total, i = sum(times), 0
    print(f"\nper-stage kernel time at T = {T} (each launch timed alone, {len(times)} launches, sum {total:.3f} ms):")
    for name, n in STAGES:
        t, m = sum(times[i:i + n]), sum(macs[i:i + n])
        tf = 2 * m / (t * 1e-3) / 1e12
        print(f"    {name:48s} {n:3d} launches {t:7.3f} ms = {100 * t / total:4.1f} %   {m / 1e9:6.2f} GMAC  {tf:6.2f} TFLOP/s = "
              f"{100 * tf / PEAK_TFLOPS:4.1f} % of peak")
        i += n


def miopen(T, crops, rounds):
    sd = {k: v.cuda() for k, v in R.seeded_state(0).items()}
    x = R.standardize(crops.permute(0, 3, 1, 2).float())
    with torch.no_grad():
        s = alternate({"torch": lambda: R.forward(sd, x)}, rounds, 3)["torch"]
    print(f"torch restatement (MIOpen) T = {T} at 128 x 128: {fmt(s)}  {T / (s['median'] * 1e-3):9.0f} faces/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-miopen", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("facenet_bench.py needs a GPU")
    L.get()
    model = mintime_amd.InceptionResnetV1()
    model.load_state_dict(R.seeded_state(0))
    model = model.cuda().eval()
    print(f"FaceNet InceptionResnetV1 on {torch.cuda.get_device_name(0)}; {a.rounds} windows per figure, median (min, max)")
    crops = None
    for T in (200, 800):
        c = whole_network(model, T, a.rounds)
        crops = crops if crops is not None else c
    print("\nfive heaviest layer shapes at T = 200 (variants alternate window by window):")
    worst = []
    for key, (macs, uses) in heaviest_layers(model, 200):
        worst.append(layer(key, macs, uses, 200, a.rounds))
    slower = [r for r, spread in worst if r > 1.0 + spread]
    print(f"\nmt_conv2d_fwd slower than mt_conv3d_fwd + pass beyond the spread on {len(slower)} of {len(worst)} shapes")
    stages(model, 200, a.rounds)
    sys.stdout.flush()
    if not a.no_miopen:
        print()
        miopen(200, crops, a.rounds)


if __name__ == "__main__":
    main()
