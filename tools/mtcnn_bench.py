#!/usr/bin/env python3
"""What the MTCNN detector costs on the device (mintime_amd.MTCNN, csrc/mtcnn.hip): 32 frames of 960 x 540 -- the reference's
batch of half-resolution 1080p frames (preprocessing/face_detector.py) -- with seeded weights (tests/mtcnn_ref.healthy_weights),
timed with device events, warm, as the median (with min and max) of `--rounds` windows of back-to-back calls; variants alternate
window by window.  Thresholds are picked on the device's own scores so that about 10^2 candidates per frame reach R-Net and a few
faces per frame leave O-Net; the counts are printed.

  (a) `detect_device` as a whole;
  (b) its parts, each re-issued alone on the buffers the last whole call left: the fused P-Net launch of every pyramid level
      (with the multiply-adds of the level and the rate against the 157.3 TFLOP/s fp32 peak), the NMS launches, crop + R-Net +
      score, crop + O-Net + score;
  (c) the plain-torch restatement of the same detector on the same device (tests/mtcnn_ref.py in fp32: MIOpen convolutions and its
      own host synchronisations: nonzero, Python NMS loops) -- the comparison; the parent of this detector has none.

Prints a text report (profiles/mtcnn_detect.txt is one run of it).

    python tools/mtcnn_bench.py --rounds 5
"""
import argparse
import os
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "2")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mintime_amd  # noqa: E402
from mintime_amd import lib as L  # noqa: E402
from mintime_amd import mtcnn_engine as E  # noqa: E402
from tests import mtcnn_ref as R  # noqa: E402

PEAK_TFLOPS = 157.3
SEED = 20


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
    return e0.elapsed_time(e1) / calls


def alternate(fns, rounds, calls):
    for fn in fns.values():
        window(fn, max(2, calls // 4))
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, calls))
    return {k: {"median": median(v), "min": min(v), "max": max(v)} for k, v in out.items()}


def fmt(s):
    return f"{s['median']:9.4f} ms (min {s['min']:.4f}, max {s['max']:.4f})"


def pnet_macs(hs, ws):
    """Multiply-adds of P-Net on one hs x ws level: conv1, conv2, conv3, the two heads."""
    c1h, c1w = hs - 2, ws - 2
    ph, pw = -(-c1h // 2), -(-c1w // 2)
    return c1h * c1w * 270 + (ph - 2) * (pw - 2) * 1440 + (ph - 4) * (pw - 4) * (4608 + 192)


def pick_thresholds(det, frames, per_frame=(250, 10, 3)):
    """Thresholds from the device's own scores: about per_frame[0] raw P-Net candidates, per_frame[1] boxes kept by R-Net and
    per_frame[2] by O-Net, per frame."""
    eng = det.engine()
    N, H, W, _ = frames.shape
    probs = []
    for s in E.pyramid_scales(H, W, det.min_face_size, det.factor):
        hs, ws = E.level_size(H, W, s)
        maps = torch.empty(N, 5, E.map_size(hs), E.map_size(ws), device="cuda")
        rec, cnt, err = torch.empty(N, 1, E.REC, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32,
                                                                                                                              device="cuda")
        L.mt.mtcnn_pnet(frames, N, H, W, hs, ws, s, 0, 1, eng.weights()["pnet"], 2.0, rec, cnt, 1, err, None, maps)
        probs.append(maps[:, 0].reshape(-1))
    probs = torch.cat(probs).sort(descending=True).values
    t = [float(0.5 * (probs[per_frame[0] * N - 1] + probs[per_frame[0] * N])), 0.0, 0.0]
    for stage, name in ((1, "stage2"), (2, "stage3")):
        det.thresholds = list(t)
        eng.debug = {}
        det.detect_device(frames)
        rec, cnt = eng.debug[name]
        eng.debug = None
        sc = torch.cat([rec[n, :int(cnt[n]), 4] for n in range(N)]).sort(descending=True).values
        k = min(per_frame[stage] * N, len(sc) - 1)
        t[stage] = float(0.5 * (sc[k - 1] + sc[k]))
    det.thresholds = list(t)
    L.zero_(eng.err)                                 # the probing calls above may have overflowed max_refined
    torch.cuda.synchronize()
    return t


def stage_counts(det, frames):
    eng = det.engine()
    eng.debug = {}
    out = det.detect_device(frames)
    out.raise_on_error()
    dbg, eng.debug = eng.debug, None
    N = frames.shape[0]
    return {"P-Net candidates": float(dbg["cand"][1].sum()) / N, "into R-Net (after both NMS)": float(dbg["stage1"][1].sum()) / N,
            "into O-Net": float(dbg["stage2"][1].sum()) / N, "faces out": float(out.count) / N}


def parts(det, frames, rounds):
    eng = det.engine()
    N, H, W, _ = frames.shape
    st = eng.state(frames.device, N, H, W)
    mt, stream = L.mt, L.stream_ptr()
    cap, cap3, levels = st["cap"], st["cap3"], st["levels"]
    Lv, pn, t = len(levels), eng.weights()["pnet"], det.thresholds
    saved = st["cnt"].clone()

    def level(l):
        hs, ws, s = levels[l]

        def fn():
            L.zero_(st["cnt1"])
            mt.mtcnn_pnet(frames, N, H, W, hs, ws, s, l, Lv, pn, t[0], st["rec1"], st["cnt1"], cap, eng.err, None, None, stream)
        return fn

    def nms():
        L.zero_(st["cntA"])
        mt.mtcnn_nms(st["rec1"], st["cnt1"], N * Lv, cap, Lv, 0, 0.5, st["recA"], st["cntA"], cap, None, eng.err, 2, stream)
        mt.mtcnn_nms(st["recA"], st["cntA"], N, cap, 1, 0, 0.7, st["recB"], st["cntB"], cap, None, eng.err, 2, stream)
        mt.mtcnn_boxes(st["recB"], st["cntB"], N, cap, 1, H, W, st["winB"], stream)

    def rnet():
        mt.mtcnn_crop(frames, N, H, W, st["winB"], st["cntB"], cap, 24, st["x24"], stream)
        head = eng._run_net(st["rnet"], stream)
        mt.mtcnn_score(head, 8, st["recA"], st["winB"], st["cntB"], N, cap, H, W, t[1], stream)       # into a list nothing reads

    def onet():
        mt.mtcnn_crop(frames, N, H, W, st["winC"], st["cntC"], cap3, 48, st["x48"], stream)
        head = eng._run_net(st["onet"], stream)
        mt.mtcnn_score(head, 8, st["recD"], st["winC"], st["cntC"], N, cap3, H, W, t[2], stream)

    det.detect_device(frames)
    print(f"\nparts of one call, each re-issued alone ({rounds} windows):")
    total_macs, total_ms = 0, 0.0
    for l, (hs, ws, s) in enumerate(levels):
        r = alternate({"x": level(l)}, rounds, 20)["x"]
        macs = N * pnet_macs(hs, ws)
        tf = 2 * macs / (r["median"] * 1e-3) / 1e12
        total_macs, total_ms = total_macs + macs, total_ms + r["median"]
        print(f"    P-Net level {l}: {hs:3d} x {ws:3d}, scale {s:.4f}  {fmt(r)}  {macs / 1e9:7.3f} GMAC  {tf:6.2f} TFLOP/s = "
              f"{100 * tf / PEAK_TFLOPS:4.1f} % of the fp32 peak")
    tf = 2 * total_macs / (total_ms * 1e-3) / 1e12
    print(f"    P-Net, all {Lv} levels: {total_ms:9.4f} ms  {total_macs / 1e9:7.3f} GMAC = {total_macs / N / 1e9:.3f} per frame  {tf:6.2f} TFLOP/s = "
          f"{100 * tf / PEAK_TFLOPS:4.1f} % of the fp32 peak (the level resample and the candidate append are inside these launches)")
    det.detect_device(frames)                        # the lists of a whole call again
    for name, fn in (("NMS 0.5 per (image, level) + NMS 0.7 per image + refine/rerec/pad", nms), (f"crop 24 + R-Net over {N * cap} rows + score", rnet),
                     (f"crop 48 + O-Net over {N * cap3} rows + score", onet)):
        print(f"    {name}: {fmt(alternate({'x': fn}, rounds, 10)['x'])}")
    st["cnt"].copy_(saved)
    L.zero_(eng.err)


def torch_restatement(frames, sd, thresholds, rounds):
    sd_dev = {k: v.float().cuda() for k, v in sd.items()}

    def run():
        return detect_face_device(frames, sd_dev, thresholds)
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median": median(times), "min": min(times), "max": max(times)}, out


def detect_face_device(frames, sd, thresholds):
    """tests/mtcnn_ref.detect_face with the tensors on the device: the networks and the resampling run there (MIOpen / ATen), the
    post-processing as the package has it -- nonzero, then NMS and the box arithmetic on the host."""
    N, H, W, _ = frames.shape
    x = frames.permute(0, 3, 1, 2).float()
    t0, t1, t2 = thresholds
    per_image = [[] for _ in range(N)]
    for lv, s in enumerate(R.pyramid_scales(H, W)):
        level = R.normalise(torch.nn.functional.interpolate(x, size=(int(H * s + 1), int(W * s + 1)), mode="area"))
        prob, reg = R.pnet_forward(sd, level)
        idx = torch.nonzero(prob >= t0)
        n_, y_, x_ = idx[:, 0], idx[:, 1], idx[:, 2]
        score, rg, key = prob[n_, y_, x_].cpu(), reg[n_, :, y_, x_].cpu(), ((lv << 24) | (y_ * prob.shape[2] + x_)).cpu()
        box, n_ = R.candidate_boxes(x_.cpu(), y_.cpu(), s), n_.cpu()
        for n in range(N):
            m = torch.nonzero(n_ == n).reshape(-1)
            keep = R.nms(box[m], score[m], key[m], 0.5, 0)
            per_image[n].append((box[m][keep], score[m][keep], rg[m][keep], key[m][keep]))
    faces = []
    for n in range(N):
        box, score, rg, key = (torch.cat([p[i] for p in per_image[n]]) for i in range(4))
        keep = R.nms(box, score, key, 0.7, 0)
        box, key = R.rerec(R.refine(box[keep], rg[keep], 0)), key[keep]
        for size, fwd, thr, form in ((24, R.rnet_forward, t1, 0), (48, R.onet_forward, t2, 1)):
            win = R.pad(box, H, W)
            ok = (win[:, 3] > win[:, 1] - 1) & (win[:, 2] > win[:, 0] - 1)
            box, key, win = box[ok], key[ok], win[ok]
            if len(box) == 0:
                break
            im = torch.cat([R.normalise(torch.nn.functional.interpolate(x[n:n + 1, :, y - 1:ey, xx - 1:ex], size=(size, size), mode="area"))
                            for xx, y, ex, ey in win.tolist()])
            prob, rg = (t.cpu() for t in fwd(sd, im))
            ip = prob > thr
            box, score, key, rg = box[ip], prob[ip], key[ip], rg[ip]
            if form == 0:
                keep = R.nms(box, score, key, 0.7, 0)
                box, score, key = R.rerec(R.refine(box[keep], rg[keep], 1)), score[keep], key[keep]
            else:
                box = R.refine(box, rg, 1)
                keep = R.nms(box, score, key, 0.7, 1)
                box, score, key = box[keep], score[keep], key[keep]
        faces.append(len(box))
    return faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mtcnn_bench.py needs a GPU")
    L.get()
    sd = R.healthy_weights(SEED)
    det = mintime_amd.MTCNN(device="cuda", max_candidates=256, max_refined=64, max_faces=8 * a.frames)
    det.load_state_dict({k: v.float() for k, v in sd.items()})
    frames = R.make_frames(SEED, a.frames, a.height, a.width).cuda()
    print(f"MTCNN detector on {torch.cuda.get_device_name(0)}: {a.frames} frames of {a.width} x {a.height}, seeded weights; {a.rounds} windows "
          "per figure, median (min, max)")
    t = pick_thresholds(det, frames)
    print(f"thresholds {t[0]:.5f}, {t[1]:.5f}, {t[2]:.5f}; capacities max_candidates = {det.max_candidates}, max_refined = {det.max_refined}, "
          f"max_faces = {det.max_faces}")
    print("per frame: " + ", ".join(f"{k} {v:.1f}" for k, v in stage_counts(det, frames).items()))
    whole = alternate({"detect_device": lambda: det.detect_device(frames)}, a.rounds, 10)["detect_device"]
    print(f"\ndetect_device, whole call: {fmt(whole)} = {whole['median'] / a.frames:.4f} ms per frame, {a.frames / (whole['median'] * 1e-3):.0f} frames/s")
    parts(det, frames, a.rounds)
    sys.stdout.flush()
    if not a.no_torch:
        r, faces = torch_restatement(frames, sd, t, max(2, a.rounds // 2))
        mine = det.detect_device(frames).image_counts.tolist()
        print(f"\ntorch restatement on the device (MIOpen + host post-processing), host clock around a synchronised call: {fmt(r)}"
              f" = {r['median'] / whole['median']:.1f} x detect_device")
        print(f"faces per frame agree with detect_device on {sum(int(a_ == b_) for a_, b_ in zip(faces, mine))} of {len(mine)} frames "
              "(fp32 on both sides, different summation orders: a flipped threshold decision is possible)")


if __name__ == "__main__":
    main()
