"""Host restatements of the two rules csrc/face_crops.hip implements, in numpy and integer arithmetic (shared by the CPU and GPU tests):

  pil_resize_u8   Pillow's 8-bit antialiased bilinear resize (what torchvision's Resize does to a PIL image), byte for byte
  crop_rect       detector box -> padded, squared, clamped window of the frame (the crop rule of the reference's predict.py)

Both are written from the rule as include/mintime_hip.h states it; the tests compare the first with Pillow itself and the second with
the reference's arithmetic run on a coordinate-coded frame."""
import math

import numpy as np

PRECISION_BITS = 22            # fractional bits of an integer coefficient
MAX_SIDE = 4096                # longest window side the kernels take


def axis_coefficients(n_in: int, n_out: int):
    """(first [n_out], count [n_out], coeff [n_out, ksize] int64) of one axis: output index i is
    clip((2^21 + sum_j src[first[i] + j] * coeff[i, j]) >> 22, 0, 255) over j < count[i]."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(math.ceil(support)) + 1
    first = np.zeros(n_out, dtype=np.int64)
    count = np.zeros(n_out, dtype=np.int64)
    coeff = np.zeros((n_out, ksize), dtype=np.int64)
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - lo
        w = np.maximum(1.0 - np.abs((np.arange(lo, lo + n) - center + 0.5) / fs), 0.0)
        total = np.cumsum(w)[-1]                     # summed in index order (np.sum adds pairwise)
        if total != 0.0:
            w = w / total
        first[i], count[i] = lo, n
        coeff[i, :n] = (w * float(1 << PRECISION_BITS) + 0.5).astype(np.int64)      # weights are >= 0: truncation rounds half up
    return first, count, coeff


def _dense(n_in, n_out):
    first, count, coeff = axis_coefficients(n_in, n_out)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        m[i, first[i]:first[i] + count[i]] = coeff[i, :count[i]]
    return m


def _pass(m, x):
    """One pass along axis 0 of x (uint8): every product and sum is an integer below 2^31, so the fp64 matmul is exact."""
    acc = (m @ x.reshape(x.shape[0], -1).astype(np.float64)).astype(np.int64) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8).reshape((m.shape[0],) + x.shape[1:])


def pil_resize_u8(img, oh: int = 128, ow: int = 128):
    """img uint8 [h, w, C] -> uint8 [oh, ow, C]: the horizontal pass into uint8 first, the vertical pass over that.  One exception,
    which Image.resize makes itself (the Python method, as of Pillow 12.2.0): a source more than 100 times as tall as wide that gets shorter is resized
    vertically first."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] >= 1 and img.shape[1] >= 1
    h, w, _ = img.shape
    if vertical_first(h, w, oh):
        mid = _pass(_dense(h, oh), img)                                            # [oh, w, C]
        return _pass(_dense(w, ow), mid.transpose(1, 0, 2)).transpose(1, 0, 2)
    mid = _pass(_dense(w, ow), img.transpose(1, 0, 2)).transpose(1, 0, 2)          # [h, ow, C]
    return _pass(_dense(h, oh), mid)


def vertical_first(h: int, w: int, oh: int) -> bool:
    return h > 100 * w and oh < h


def _floor_div(a, b):
    return a // b              # Python's // floors, also for negative a


def crop_rect(box, H: int, W: int, max_side: int = MAX_SIDE):
    """box = (xmin, ymin, xmax, ymax) in half-resolution coordinates -> (x0, y0, w, h, valid) in the H x W frame; an invalid box is
    (0, 0, 0, 0, 0).  Invalid: an empty window, a window whose far end would be a negative slice stop, a side above max_side."""
    doubled = [float(np.float32(b) * np.float32(2)) for b in box]
    if not all(abs(v) <= float(1 << 29) for v in doubled):                          # NaN, infinities, absurd coordinates
        return 0, 0, 0, 0, 0
    x_lo, y_lo, x_hi, y_hi = (int(v) for v in doubled)                              # truncates toward zero
    w, h = x_hi - x_lo, y_hi - y_lo
    pad_h, pad_w = _floor_div(h, 3), _floor_div(w, 3)
    span_h = (y_hi + pad_h) - max(y_lo - pad_h, 0)
    span_w = (x_hi + pad_w) - max(x_lo - pad_w, 0)
    if span_h > span_w:
        pad_h -= (span_h - span_w) // 2              # the difference is positive here: // is the truncation
    else:
        pad_w -= (span_w - span_h) // 2
    y0, y1 = max(y_lo - pad_h, 0), y_hi + pad_h
    x0, x1 = max(x_lo - pad_w, 0), x_hi + pad_w
    if y1 < 0 or x1 < 0:
        return 0, 0, 0, 0, 0
    y1, x1 = min(y1, H), min(x1, W)
    ch, cw = y1 - y0, x1 - x0
    if ch <= 0 or cw <= 0:
        return 0, 0, 0, 0, 0
    if ch > cw:                                      # the window met an edge: trim the long side back towards square
        d = (ch - cw) // 2
        if d > 0:
            y0, ch = y0 + d, ch - 2 * d
        else:
            y0, ch = y0 + 1, ch - 1
    elif ch < cw:
        d = (cw - ch) // 2
        if d > 0:
            x0, cw = x0 + d, cw - 2 * d
        else:
            cw -= 1
    if ch > max_side or cw > max_side:
        return 0, 0, 0, 0, 0
    return x0, y0, cw, ch, 1


# The frames-entry cases of the tests: boxes (half-resolution coordinates) for frames of FRAME_H x FRAME_W.
FRAME_H, FRAME_W = 360, 480
BOXES = [
    ("interior", (60.0, 40.0, 100.0, 90.0)),
    ("left edge", (0.0, 50.0, 30.0, 90.0)),
    ("top edge", (100.0, 0.0, 140.0, 45.0)),
    ("right edge", (200.0, 60.0, 240.0, 110.0)),
    ("bottom edge", (90.0, 140.0, 130.0, 180.0)),
    ("negative near corner", (-5.5, -3.25, 30.0, 40.0)),
    ("beyond the far corner", (210.0, 150.0, 260.0, 200.0)),
    ("beyond the right edge only", (225.5, 70.0, 251.0, 99.0)),
    ("tall and thin", (100.0, 20.0, 104.0, 160.0)),
    ("wide and flat", (20.0, 80.0, 220.0, 84.0)),
    ("one row too many", (60.0, 40.0, 100.0, 90.5)),
    ("one column too many", (60.0, 40.0, 100.5, 80.0)),
    ("one pixel wide", (50.0, 50.0, 50.5, 80.0)),
    ("fractional", (33.7, 21.2, 77.9, 80.4)),
    ("large", (10.0, 5.0, 230.0, 175.0)),
    ("empty", (50.0, 50.0, 50.0, 50.0)),
    ("negative far end", (-40.0, 10.0, -20.0, 30.0)),
    ("inverted", (120.0, 60.0, 100.0, 30.0)),
    ("not a number", (float("nan"), 10.0, 60.0, 70.0)),
    ("outside the frame", (300.0, 200.0, 340.0, 250.0)),
]
