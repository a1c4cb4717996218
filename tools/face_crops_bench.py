#!/usr/bin/env python3
"""What cutting and resizing the face crops costs on the device: `FaceCropPlan.run` (mt_face_rects + mt_crop_resize_u8,
csrc/face_crops.hip) and `FaceCropPlan.run_ragged` on the same crops, timed with device events, warm, as the median (with min and
max) of `--rounds` windows of `--calls` back-to-back calls, for 200 and 800 faces cut from eight 1080p frames with window sides
spread over 60 to 600 pixels.  Beside them, in the same process:

  host      the reference's own path on this host's CPU: numpy slice, Pillow `resize((128, 128), BILINEAR)`, np.stack, upload
            (wall clock, one warm run and the median of three); its bytes are compared with the kernel's
  torch     a per-crop `F.interpolate(mode="bilinear", antialias=True)` loop on the device (float arithmetic: not byte-equal to
            Pillow; the count of differing bytes is reported)
  embedder  `InceptionResnetV1.embed_crops` on the same faces (seeded weights), to put the crop time beside what consumes it

Prints one JSON line.

    python tools/face_crops_bench.py --rounds 7 --calls 50
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mintime_amd  # noqa: E402
from mintime_amd import FaceCropPlan, lib  # noqa: E402
from tests import facenet_ref  # noqa: E402

H, W, FRAMES = 1080, 1920, 8


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def events(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # microseconds per call


def windows(fn, rounds, calls):
    events(fn, max(5, calls // 10))                   # warm: code objects loaded, clocks up
    v = [events(fn, calls) for _ in range(rounds)]
    return {"median_us": round(median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def boxes_for(rng, T):
    """Detector boxes (half-resolution coordinates) whose padded windows have sides spread evenly over 60..600 pixels."""
    side = np.linspace(60, 600, T)[rng.permutation(T)]
    half = side * 0.3                                 # a box of b half-resolution pixels becomes a window of about 2 b (1 + 2/3)
    cx = rng.uniform(half / 2, W / 2 - half / 2)
    cy = rng.uniform(half / 2, H / 2 - half / 2)
    aspect = rng.uniform(0.8, 1.25, T)
    bw, bh = half * np.sqrt(aspect), half / np.sqrt(aspect)
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=1).astype(np.float32)


def measure(T, frames_host, frames, model, a):
    rng = np.random.default_rng(T)
    boxes_host = boxes_for(rng, T)
    index_host = rng.integers(0, FRAMES, T).astype(np.int32)
    boxes, index = torch.from_numpy(boxes_host).cuda(), torch.from_numpy(index_host).cuda()
    plan = FaceCropPlan(T)
    res = plan.run(frames, boxes, index).raise_on_error()
    rects = res.rects.cpu().numpy()
    got = res.crops.cpu().numpy()
    src_bytes = int((rects[:, 2].astype(np.int64) * rects[:, 3] * 3).sum())
    out = {"faces": T, "window_side_px": [int(rects[:, 2:].min()), int(rects[:, 2:].max())], "source_bytes": src_bytes}

    out["frames_entry"] = windows(lambda: plan.run(frames, boxes, index), a.rounds, a.calls)
    out["frames_entry"]["source_GB_per_s"] = round(src_bytes / out["frames_entry"]["median_us"] / 1e3, 1)
    out["rects_alone"] = windows(lambda: lib.mt.face_rects(boxes, index, T, FRAMES, H, W, plan.rects, plan.valid, plan.err),
                                 a.rounds, a.calls)

    images = [frames[f, y:y + h, x:x + w].contiguous() for (x, y, w, h), f in zip(rects.tolist(), index_host.tolist())]
    ragged_plan = FaceCropPlan(T)
    same = bool(torch.equal(ragged_plan.run_ragged(images).crops, res.crops))
    out["ragged_entry"] = windows(lambda: ragged_plan.run_ragged(images), a.rounds, max(5, a.calls // 5))
    out["ragged_entry"]["equals_frames_entry"] = same

    # the reference's host path on this CPU
    try:
        from PIL import Image

        def host_path():
            faces = []
            for (x, y, w, h), f in zip(rects.tolist(), index_host.tolist()):
                faces.append(np.uint8(Image.fromarray(frames_host[f, y:y + h, x:x + w]).resize((128, 128), Image.BILINEAR)))
            return torch.as_tensor(np.stack(faces)).cuda()

        host_path()
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            up = host_path()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out["host_pillow_path_ms"] = round(median(times), 2)
        out["bytes_equal_pillow"] = bool(np.array_equal(up.cpu().numpy(), got))
    except ImportError:
        out["host_pillow_path_ms"] = None

    # torch-ROCm restatement: one antialiased interpolate per crop
    def torch_path():
        faces = [F.interpolate(im.permute(2, 0, 1)[None].float(), size=(128, 128), mode="bilinear", antialias=True, align_corners=False)
                 for im in images]
        return torch.cat(faces).round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)

    tp = torch_path()
    diff = (tp.cpu().numpy().astype(np.int16) - got).astype(np.int16)
    out["torch_interpolate_loop"] = windows(torch_path, max(3, a.rounds // 2), max(3, a.calls // 10))
    out["torch_interpolate_loop"]["bytes_differing_from_pillow"] = int((diff != 0).sum())
    out["torch_interpolate_loop"]["max_abs_difference"] = int(np.abs(diff).max())

    out["embed_crops"] = windows(lambda: model.embed_crops(res.crops), max(3, a.rounds // 2), max(3, a.calls // 10))
    out["share_of_embed_crops"] = round(out["frames_entry"]["median_us"] / out["embed_crops"]["median_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("face_crops_bench.py needs a GPU")
    lib.get()
    frames_host = np.random.default_rng(0).integers(0, 256, (FRAMES, H, W, 3), dtype=np.uint8)
    frames = torch.from_numpy(frames_host).cuda()
    model = mintime_amd.InceptionResnetV1()
    model.load_state_dict(facenet_ref.seeded_state(0))
    model = model.cuda().eval()
    out = {"frames": f"{FRAMES} x {H} x {W}", "rounds": a.rounds, "calls_per_window": a.calls, "host_cpus": os.cpu_count()}
    for T in (200, 800):
        out[f"faces_{T}"] = measure(T, frames_host, frames, model, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
