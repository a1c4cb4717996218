"""Plain-torch restatement of the MTCNN detector as include/mintime_hip.h states it (facenet_pytorch's detect_face with the four
defined deviations), on the CPU, in fp64 or fp32.  It returns every intermediate -- levels, maps, candidate lists, picks, boxes per
stage -- and the SMALLEST DECISION MARGIN of the run: the minimum over |score - t| of every thresholded score, |overlap - thr| of
every compared pair with a non-integer operand, and the distance to the nearest integer of every truncated non-integer coordinate.
A run whose margin is far above the arithmetic error of a second implementation takes the same decisions there.

The candidate box of a map position, floor((2x + 1) / s) ..., is fp32 arithmetic on exact operands by definition (the package's
own), so it is computed in fp32 whatever `dtype` is and its floors are not decisions of precision (at s = 0.6 a third of the
quotients are integers in exact arithmetic and fall to either side in fp32 and fp64).

Also here: seeded "healthy" weights (He-scaled, heads widened so the probabilities spread over (0, 1)), smooth-plus-noise frames
(pure noise averages to grey under area resampling), and the generator of tests/golden/mtcnn_case.npz (`python tests/mtcnn_ref.py`).
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = {
    "pnet": [("conv1", (10, 3, 3, 3)), ("prelu1", (10,)), ("conv2", (16, 10, 3, 3)), ("prelu2", (16,)), ("conv3", (32, 16, 3, 3)),
             ("prelu3", (32,)), ("conv4_1", (2, 32, 1, 1)), ("conv4_2", (4, 32, 1, 1))],
    "rnet": [("conv1", (28, 3, 3, 3)), ("prelu1", (28,)), ("conv2", (48, 28, 3, 3)), ("prelu2", (48,)), ("conv3", (64, 48, 2, 2)),
             ("prelu3", (64,)), ("dense4", (128, 576)), ("prelu4", (128,)), ("dense5_1", (2, 128)), ("dense5_2", (4, 128))],
    "onet": [("conv1", (32, 3, 3, 3)), ("prelu1", (32,)), ("conv2", (64, 32, 3, 3)), ("prelu2", (64,)), ("conv3", (64, 64, 3, 3)),
             ("prelu3", (64,)), ("conv4", (128, 64, 2, 2)), ("prelu4", (128,)), ("dense5", (256, 1152)), ("prelu5", (256,)),
             ("dense6_1", (2, 256)), ("dense6_2", (4, 256)), ("dense6_3", (10, 256))],
}


def manifest():
    """{state-dict key: shape} of the package's MTCNN (pnet. / rnet. / onet. prefixes)."""
    out = {}
    for net, layers in SHAPES.items():
        for name, shape in layers:
            out[f"{net}.{name}.weight"] = list(shape)
            if not name.startswith("prelu"):
                out[f"{net}.{name}.bias"] = [shape[0]]
    return out


def healthy_weights(seed):
    """A state dict (fp64) with the manifest's keys: He-scaled filters, small biases, PReLU slopes around 0.25, the class heads
    widened to logit differences of a few units and the regression heads narrowed to a fraction of a box."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for net, layers in SHAPES.items():
        for name, shape in layers:
            if name.startswith("prelu"):
                sd[f"{net}.{name}.weight"] = 0.25 + 0.1 * torch.rand(shape, generator=g, dtype=torch.float64)
                continue
            fan_in = int(np.prod(shape[1:]))
            gain = math.sqrt(2.0 / fan_in)
            if name.endswith("_1"):
                gain *= 3.0
            elif name.endswith("_2"):
                gain *= 0.15
            sd[f"{net}.{name}.weight"] = gain * torch.randn(shape, generator=g, dtype=torch.float64)
            sd[f"{net}.{name}.bias"] = 0.05 * torch.randn(shape[0], generator=g, dtype=torch.float64)
    return sd


def make_frames(seed, N, H, W):
    """[N, H, W, 3] uint8: a smooth random field (so every pyramid level keeps contrast) plus pixel noise."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(N, 3, max(H // 12, 2), max(W // 12, 2), generator=g)
    smooth = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)
    x = 255.0 * (0.15 + 0.7 * smooth) + 12.0 * torch.randn(N, 3, H, W, generator=g)
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pyramid_scales(H, W, minsize=20, factor=0.709):
    m = 12.0 / minsize
    minl = min(H, W) * m
    s, out = m, []
    while minl >= 12:
        out.append(s)
        s = s * factor
        minl = minl * factor
    return out


def area_matrix(n_in, n_out, dtype):
    """[n_out, n_in]: 1 where source index j belongs to output cell i (floor(i in / out) .. ceil((i + 1) in / out) - 1)."""
    a = torch.zeros(n_out, n_in, dtype=dtype)
    for i in range(n_out):
        a[i, (i * n_in) // n_out: -((-(i + 1) * n_in) // n_out)] = 1
    return a


def area_resize(x, oh, ow):
    """x [N, C, H, W] -> [N, C, oh, ow]: every output cell the mean of its source cells (sum first, one division)."""
    ay, ax = area_matrix(x.shape[2], oh, x.dtype), area_matrix(x.shape[3], ow, x.dtype)
    s = torch.einsum("ih,nchw,jw->ncij", ay, x, ax)
    return s / (ay.sum(1)[:, None] * ax.sum(1)[None, :])


def normalise(x):
    return (x - 127.5) * 0.0078125


def _sd(sd, net, dtype):
    return {k[len(net) + 1:]: v.to(dtype) for k, v in sd.items() if k.startswith(net + ".")}


def pnet_forward(sd, x):
    """x [N, 3, Hs, Ws] -> prob [N, Hm, Wm], reg [N, 4, Hm, Wm]"""
    p = _sd(sd, "pnet", x.dtype)
    x = F.prelu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"]), p["prelu1.weight"])
    x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    x = F.prelu(F.conv2d(x, p["conv2.weight"], p["conv2.bias"]), p["prelu2.weight"])
    x = F.prelu(F.conv2d(x, p["conv3.weight"], p["conv3.bias"]), p["prelu3.weight"])
    a = torch.softmax(F.conv2d(x, p["conv4_1.weight"], p["conv4_1.bias"]), dim=1)
    return a[:, 1], F.conv2d(x, p["conv4_2.weight"], p["conv4_2.bias"])


def flatten_whc(x):
    """The package's flatten of [N, C, H, W]: (w, h, c) order."""
    return x.permute(0, 3, 2, 1).contiguous().view(x.shape[0], -1)


def rnet_forward(sd, x):
    """x [n, 3, 24, 24] -> prob [n], reg [n, 4]"""
    p = _sd(sd, "rnet", x.dtype)
    x = F.max_pool2d(F.prelu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"]), p["prelu1.weight"]), 3, 2, ceil_mode=True)
    x = F.max_pool2d(F.prelu(F.conv2d(x, p["conv2.weight"], p["conv2.bias"]), p["prelu2.weight"]), 3, 2, ceil_mode=True)
    x = F.prelu(F.conv2d(x, p["conv3.weight"], p["conv3.bias"]), p["prelu3.weight"])
    x = F.prelu(F.linear(flatten_whc(x), p["dense4.weight"], p["dense4.bias"]), p["prelu4.weight"])
    a = torch.softmax(F.linear(x, p["dense5_1.weight"], p["dense5_1.bias"]), dim=1)
    return a[:, 1], F.linear(x, p["dense5_2.weight"], p["dense5_2.bias"])


def onet_forward(sd, x):
    """x [n, 3, 48, 48] -> prob [n], reg [n, 4]"""
    p = _sd(sd, "onet", x.dtype)
    x = F.max_pool2d(F.prelu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"]), p["prelu1.weight"]), 3, 2, ceil_mode=True)
    x = F.max_pool2d(F.prelu(F.conv2d(x, p["conv2.weight"], p["conv2.bias"]), p["prelu2.weight"]), 3, 2, ceil_mode=True)
    x = F.max_pool2d(F.prelu(F.conv2d(x, p["conv3.weight"], p["conv3.bias"]), p["prelu3.weight"]), 2, 2, ceil_mode=True)
    x = F.prelu(F.conv2d(x, p["conv4.weight"], p["conv4.bias"]), p["prelu4.weight"])
    x = F.prelu(F.linear(flatten_whc(x), p["dense5.weight"], p["dense5.bias"]), p["prelu5.weight"])
    a = torch.softmax(F.linear(x, p["dense6_1.weight"], p["dense6_1.bias"]), dim=1)
    return a[:, 1], F.linear(x, p["dense6_2.weight"], p["dense6_2.bias"])


class Margin:
    def __init__(self):
        self.value = float("inf")

    def near(self, x, t):
        """|x - t| of thresholded values"""
        if x.numel():
            self.value = min(self.value, float((x.double() - float(t)).abs().min()))

    def integer(self, x):
        """distance to the nearest integer of truncated non-integer values"""
        f = (x.double() - x.double().round()).abs().reshape(-1)
        f = f[f > 0]
        if f.numel():
            self.value = min(self.value, float(f.min()))


def candidate_boxes(x, y, s):
    """fp32 by definition: floor((2x + 1) / s), floor((2y + 1) / s), floor((2x + 12) / s), floor((2y + 12) / s)"""
    s32 = torch.tensor(s, dtype=torch.float32)
    x, y = x.to(torch.float32), y.to(torch.float32)
    return torch.stack([((2 * x + 1) / s32).floor(), ((2 * y + 1) / s32).floor(), ((2 * x + 12) / s32).floor(),
                        ((2 * y + 12) / s32).floor()], 1)


def nms(boxes, scores, keys, thr, form, margin=None):
    """Greedy NMS of one segment -> kept input rows, in order.  form 0: torchvision's union form; form 1: the package's numpy form
    with method Min.  Order: score descending, key ascending (deviation (a))."""
    n = boxes.shape[0]
    order = sorted(range(n), key=lambda i: (-float(scores[i]), int(keys[i])))
    b = boxes[order]
    one = 1 if form else 0
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    thr_t = torch.tensor(thr, dtype=boxes.dtype)
    whole = (b == b.round()).all(1)
    alive = torch.ones(n, dtype=torch.bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(order[i])
        j = torch.nonzero(alive[i + 1:]).reshape(-1) + i + 1
        if j.numel() == 0:
            continue
        w = (torch.minimum(b[i, 2], b[j, 2]) - torch.maximum(b[i, 0], b[j, 0]) + one).clamp(min=0)
        h = (torch.minimum(b[i, 3], b[j, 3]) - torch.maximum(b[i, 1], b[j, 1]) + one).clamp(min=0)
        inter = w * h
        ov = inter / (torch.minimum(area[i], area[j]) if form else area[i] + area[j] - inter)
        if margin is not None:
            part = ~(whole[i] & whole[j])
            margin.near(ov[part & ~torch.isnan(ov)], thr)
        alive[j[ov > thr_t]] = False
    return keep


def refine(boxes, reg, plus_one):
    w, h = boxes[:, 2] - boxes[:, 0] + plus_one, boxes[:, 3] - boxes[:, 1] + plus_one
    return torch.stack([boxes[:, 0] + reg[:, 0] * w, boxes[:, 1] + reg[:, 1] * h, boxes[:, 2] + reg[:, 2] * w, boxes[:, 3] + reg[:, 3] * h], 1)


def rerec(b):
    h, w = b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]
    l = torch.maximum(w, h)
    x1 = b[:, 0] + w * 0.5 - l * 0.5
    y1 = b[:, 1] + h * 0.5 - l * 0.5
    return torch.stack([x1, y1, x1 + l, y1 + l], 1)


def pad(boxes, H, W, margin=None):
    """-> int64 [n, 4] = (x, y, ex, ey)"""
    if margin is not None:
        margin.integer(boxes)
    t = boxes.trunc().to(torch.int64)
    return torch.stack([t[:, 0].clamp(min=1), t[:, 1].clamp(min=1), t[:, 2].clamp(max=W), t[:, 3].clamp(max=H)], 1)


def crops(frames_f, img, win, size):
    """frames_f [N, 3, H, W]; the windows of image `img` -> [n, 3, size, size] normalised, and ok [n] (deviation (c))."""
    out = torch.zeros(win.shape[0], 3, size, size, dtype=frames_f.dtype)
    ok = torch.zeros(win.shape[0], dtype=torch.bool)
    for k, (x, y, ex, ey) in enumerate(win.tolist()):
        if ey > y - 1 and ex > x - 1:
            out[k] = normalise(area_resize(frames_f[img:img + 1, :, y - 1:ey, x - 1:ex], size, size))[0]
            ok[k] = True
    return out, ok


def detect_face(frames, sd, thresholds, dtype=torch.float64, minsize=20, factor=0.709):
    """frames [N, H, W, 3] uint8 -> dict of every intermediate.  Per image n: stage1 / stage2 / stage3 [n] = (boxes [k, 4], scores
    [k], keys [k]) in NMS order; levels, maps, cand per level; margin."""
    N, H, W, _ = frames.shape
    x = frames.permute(0, 3, 1, 2).to(dtype)
    t0, t1, t2 = thresholds
    margin = Margin()
    out = {"levels": [], "maps": [], "cand": [], "scales": pyramid_scales(H, W, minsize, factor)}
    per_image = [[] for _ in range(N)]
    for lv, s in enumerate(out["scales"]):
        level = normalise(area_resize(x, int(H * s + 1), int(W * s + 1)))
        prob, reg = pnet_forward(sd, level)
        out["levels"].append(level)
        out["maps"].append((prob, reg))
        margin.near(prob, t0)
        idx = torch.nonzero(prob >= t0)
        n_, y_, x_ = idx[:, 0], idx[:, 1], idx[:, 2]
        cand = {"img": n_, "y": y_, "x": x_, "score": prob[n_, y_, x_], "reg": reg[n_, :, y_, x_],
                "box": candidate_boxes(x_, y_, s).to(dtype), "key": (lv << 24) | (y_ * prob.shape[2] + x_)}
        out["cand"].append(cand)
        for n in range(N):
            m = torch.nonzero(n_ == n).reshape(-1)
            keep = nms(cand["box"][m], cand["score"][m], cand["key"][m], 0.5, 0, margin)
            per_image[n].append({k: v[m][keep] for k, v in cand.items()})
    out["stage1"], out["stage2"], out["stage3"] = [], [], []
    for n in range(N):
        c = {k: torch.cat([p[k] for p in per_image[n]]) for k in per_image[n][0]}
        keep = nms(c["box"], c["score"], c["key"], 0.7, 0, margin)
        box, score, key = rerec(refine(c["box"][keep], c["reg"][keep], 0)), c["score"][keep], c["key"][keep]
        out["stage1"].append((box, score, key))
        # stage 2
        win = pad(box, H, W, margin)
        im, ok = crops(x, n, win, 24)
        prob, reg = rnet_forward(sd, im) if len(im) else (torch.zeros(0, dtype=dtype), torch.zeros(0, 4, dtype=dtype))
        margin.near(prob[ok], t1)
        ip = ok & (prob > t1)
        box, score, key, reg = box[ip], prob[ip], key[ip], reg[ip]
        keep = nms(box, score, key, 0.7, 0, margin)
        box, score, key = rerec(refine(box[keep], reg[keep], 1)), score[keep], key[keep]
        out["stage2"].append((box, score, key))
        # stage 3
        win = pad(box, H, W, margin)
        im, ok = crops(x, n, win, 48)
        prob, reg = onet_forward(sd, im) if len(im) else (torch.zeros(0, dtype=dtype), torch.zeros(0, 4, dtype=dtype))
        margin.near(prob[ok], t2)
        ip = ok & (prob > t2)
        box, score, key = refine(box[ip], reg[ip], 1), prob[ip], key[ip]
        keep = nms(box, score, key, 0.7, 1, margin)
        out["stage3"].append((box[keep], score[keep], key[keep]))
    out["margin"] = margin.value
    return out


# ---- the committed case: tests/golden/mtcnn_case.npz -------------------------------------------------------------------------
CASE_N, CASE_H, CASE_W = 2, 96, 128
CASE_WANTED = (80, 24, 8)          # candidates at stage 1, boxes kept by R-Net and by O-Net, over both frames: where the gap is sought
CASE_FACTOR = 50.0


def widest_gap(values, wanted):
    """A threshold in the widest gap of the sorted scores that leaves about `wanted` of them above it."""
    v = np.sort(np.asarray(values, dtype=np.float64))[::-1]
    if len(v) < 2:
        return 0.5
    lo, hi = max(1, wanted // 2), min(len(v) - 1, max(wanted * 3 // 2, 2))
    k = max(range(lo, hi + 1), key=lambda i: v[i - 1] - v[i]) if hi >= lo else len(v) // 2
    return float((v[k - 1] + v[k]) / 2)


def choose_thresholds(frames, sd):
    """Thresholds of the three stages, each in the widest gap of the fp64 scores near the wanted count."""
    probe = detect_face(frames, sd, (2.0, 2.0, 2.0))
    t0 = widest_gap(torch.cat([p.reshape(-1) for p, _ in probe["maps"]]).numpy(), CASE_WANTED[0])
    x = frames.permute(0, 3, 1, 2).double()
    H, W = frames.shape[1:3]
    s1 = detect_face(frames, sd, (t0, 2.0, 2.0))["stage1"]
    sc = [rnet_forward(sd, crops(x, n, pad(b, H, W), 24)[0])[0] for n, (b, _, _) in enumerate(s1) if len(b)]
    t1 = widest_gap(torch.cat(sc).numpy(), CASE_WANTED[1])
    s2 = detect_face(frames, sd, (t0, t1, 2.0))["stage2"]
    sc = [onet_forward(sd, crops(x, n, pad(b, H, W), 48)[0])[0] for n, (b, _, _) in enumerate(s2) if len(b)]
    t2 = widest_gap(torch.cat(sc).numpy(), CASE_WANTED[2])
    return t0, t1, t2


def same_decisions(a, b):
    return all(len(x[2]) == len(y[2]) and bool((x[2] == y[2]).all()) for st in ("stage1", "stage2", "stage3") for x, y in zip(a[st], b[st])) \
        and all(bool((ca["key"] == cb["key"]).all()) if len(ca["key"]) == len(cb["key"]) else False for ca, cb in zip(a["cand"], b["cand"]))


def fp32_error(r64, r32):
    """(largest score error, largest coordinate error) of the fp32 restatement against fp64; the decisions must agree."""
    es = max(float((p64 - p32.double()).abs().max()) for (p64, _), (p32, _) in zip(r64["maps"], r32["maps"]))
    ec = 0.0
    for st in ("stage1", "stage2", "stage3"):
        for x, y in zip(r64[st], r32[st]):
            if len(x[0]):
                ec = max(ec, float((x[0] - y[0].double()).abs().max()))
                es = max(es, float((x[1] - y[1].double()).abs().max()))
    return es, ec


def evaluate_seed(seed):
    frames, sd = make_frames(seed, CASE_N, CASE_H, CASE_W), healthy_weights(seed)
    thr = choose_thresholds(frames, sd)
    r64, r32 = detect_face(frames, sd, thr), detect_face(frames, sd, thr, dtype=torch.float32)
    if not same_decisions(r64, r32) or sum(len(s[0]) for s in r64["stage3"]) == 0:
        return None
    es, ec = fp32_error(r64, r32)
    return {"seed": seed, "thresholds": thr, "margin": r64["margin"], "score_err": es, "coord_err": ec,
            "factor": r64["margin"] / max(es, ec), "r64": r64}


def load_case():
    z = np.load(os.path.join(GOLDEN, "mtcnn_case.npz"))
    return {k: z[k] for k in z.files}


def write_case(seeds=range(32)):
    found = [e for e in (evaluate_seed(s) for s in seeds) if e is not None]
    best = max(found, key=lambda e: e["factor"])
    r = best["r64"]
    arrays = {"seed": np.int64(best["seed"]), "thresholds": np.asarray(best["thresholds"], np.float64), "margin": np.float64(best["margin"]),
              "score_err": np.float64(best["score_err"]), "coord_err": np.float64(best["coord_err"]),
              "factor": np.float64(min(best["factor"], CASE_FACTOR)), "achieved_factor": np.float64(best["factor"]),
              "shape": np.asarray([CASE_N, CASE_H, CASE_W], np.int64)}
    for st in ("stage1", "stage2", "stage3"):
        arrays[st + "_boxes"] = torch.cat([b for b, _, _ in r[st]]).numpy()
        arrays[st + "_scores"] = torch.cat([s for _, s, _ in r[st]]).numpy()
        arrays[st + "_keys"] = torch.cat([k for _, _, k in r[st]]).numpy()
        arrays[st + "_counts"] = np.asarray([len(k) for _, _, k in r[st]], np.int64)
    arrays["cand_counts"] = np.asarray([[int((c["img"] == n).sum()) for c in r["cand"]] for n in range(CASE_N)], np.int64)
    np.savez(os.path.join(GOLDEN, "mtcnn_case.npz"), **arrays)
    return best, found


if __name__ == "__main__":
    best, found = write_case()
    for e in found:
        print(f"seed {e['seed']:2d}  margin {e['margin']:.3e}  score err {e['score_err']:.2e}  coord err {e['coord_err']:.2e}  "
              f"factor {e['factor']:.1f}  thresholds {tuple(round(t, 5) for t in e['thresholds'])}")
    print("chosen", best["seed"], "factor", best["factor"], "counts", [[len(s[2]) for s in best["r64"][st]] for st in ("stage1", "stage2", "stage3")])
