"""The reference's SlowFast input transform (utils.py:166-186) in torch on the CPU, at a chosen dtype and differentiable with respect to
the clip: UniformTemporalSubsample -> /255 -> Normalize -> ShortSideScale -> CenterCropVideo -> PackPathway.  ShortSideScale's size rule
and CenterCropVideo's rounding are restated from pytorchvideo's and torchvision's published source (not checked against either package)."""
import math

import torch
import torch.nn.functional as F


def short_side_size(H, W, side_size):
    if W < H:
        return int(math.floor(float(H) / W * side_size)), side_size
    return side_size, int(math.floor(float(W) / H * side_size))


def transform(videos, layout, dtype, crop_size, side_size, num_frames=32, alpha=4):
    """videos [B, F, H, W, 3] ('bfhwc') or [B, 3, F, H, W] ('bcfhw'), any dtype -> [slow, fast], each [B, 3, T, crop, crop] of `dtype`.
    A floating-point `videos` of `dtype` that requires grad receives its gradient through the returned pair."""
    x = videos.to(dtype)
    x = x.permute(0, 4, 1, 2, 3) if layout == "bfhwc" else x
    x = torch.index_select(x, 2, torch.linspace(0, x.shape[2] - 1, num_frames).long())
    x = x / 255.0
    x = (x - 0.45) / 0.225
    B, C, T, H, W = x.shape
    Hr, Wr = short_side_size(H, W, side_size)
    x = F.interpolate(x.reshape(B, C * T, H, W), size=(Hr, Wr), mode="bilinear", align_corners=False).reshape(B, C, T, Hr, Wr)
    if Hr < crop_size or Wr < crop_size:
        raise ValueError("height and width must be no smaller than crop_size")
    top, left = int(round((Hr - crop_size) / 2.0)), int(round((Wr - crop_size) / 2.0))
    x = x[..., top:top + crop_size, left:left + crop_size]
    slow = torch.index_select(x, 2, torch.linspace(0, T - 1, T // alpha).long())
    return [slow, x]
