"""SlowFast R50 (reference train.py:143-147 / test.py:121-125, `--model 2`) on libmintime_hip (MI355X).

The reference loads pytorchvideo's `slowfast_r50` from the network and replaces its classifier:

    model = torch.hub.load('facebookresearch/pytorchvideo', 'slowfast_r50', pretrained=True)
    model.blocks[6].proj = torch.nn.Linear(2304, 1)

`slowfast_r50()` builds the same network from its published structure (pytorchvideo `create_slowfast`: depth 50, alpha 4, beta 1/8,
fusion kernel (7, 1, 1)) with pytorchvideo's module names, so the state-dict keys and shapes are pytorchvideo's
(tests/golden/slowfast_r50_manifest.json, written by hand from that structure: it has not been checked against pytorchvideo itself).
The modules only hold parameters and settings; `SlowFast.forward` runs the whole network in the HIP library (slowfast_engine.py).

Inputs: `forward([slow, fast])` with slow [B, 3, 8, H, W] and fast [B, 3, 32, H, W] (the reference's PackPathway output), or the pair
`slowfast_input_transform(videos)` returns (device tensors that the network reads without a copy).  Pathway tensors or fp32 videos
that require grad get their gradient through autograd (the stems' data gradient mt_sf_stem_dgrad, the ingest's adjoint
mt_sf_ingest_bwd, or mt_sf_ingest_resize_bwd when the transform resizes and crops); without one nothing is recorded and the packing
reads `x.detach()`.
"""
import math

import torch
from torch import nn

from . import lib as L

SLOW_INNER = (64, 128, 256, 512)
SLOW_OUT = (256, 512, 1024, 2048)
FAST_INNER = (8, 16, 32, 64)
FAST_OUT = (32, 64, 128, 256)
DEPTHS = (3, 4, 6, 3)
SLOW_CONV_A_T = (1, 1, 3, 3)
FAST_CONV_A_T = (3, 3, 3, 3)
STAGE_STRIDE = (1, 2, 2, 2)
STEM_OUT = (64, 8)
FUSION_KERNEL, FUSION_STRIDE, FUSION_RATIO = 7, 4, 2
ALPHA = 4                                   # fast frames per slow frame (PackPathway)
HEAD_DIM = SLOW_OUT[-1] + FAST_OUT[-1]      # 2304
NUM_FRAMES = 32                             # UniformTemporalSubsample(32) of utils.py:166


class _Stem(nn.Module):
    def __init__(self, cout, kt):
        super().__init__()
        self.conv = nn.Conv3d(3, cout, (kt, 7, 7), stride=(1, 2, 2), padding=(kt // 2, 3, 3), bias=False)
        self.norm = nn.BatchNorm3d(cout, eps=1e-5, momentum=0.1)
        self.activation = nn.ReLU()
        self.pool = nn.MaxPool3d((1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))


class _Fusion(nn.Module):
    def __init__(self, cfast):
        super().__init__()
        cout = FUSION_RATIO * cfast
        self.conv_fast_to_slow = nn.Conv3d(cfast, cout, (FUSION_KERNEL, 1, 1), stride=(FUSION_STRIDE, 1, 1),
                                           padding=(FUSION_KERNEL // 2, 0, 0), bias=False)
        self.norm = nn.BatchNorm3d(cout, eps=1e-5, momentum=0.1)
        self.activation = nn.ReLU()


class _Branch2(nn.Module):
    def __init__(self, cin, inner, cout, kt, stride):
        super().__init__()
        self.conv_a = nn.Conv3d(cin, inner, (kt, 1, 1), padding=(kt // 2, 0, 0), bias=False)
        self.norm_a = nn.BatchNorm3d(inner, eps=1e-5, momentum=0.1)
        self.act_a = nn.ReLU()
        self.conv_b = nn.Conv3d(inner, inner, (1, 3, 3), stride=(1, stride, stride), padding=(0, 1, 1), bias=False)
        self.norm_b = nn.BatchNorm3d(inner, eps=1e-5, momentum=0.1)
        self.act_b = nn.ReLU()
        self.conv_c = nn.Conv3d(inner, cout, 1, bias=False)
        self.norm_c = nn.BatchNorm3d(cout, eps=1e-5, momentum=0.1)
        self.norm_c.block_final_bn = True


class _ResBlock(nn.Module):
    def __init__(self, cin, inner, cout, kt, stride):
        super().__init__()
        if cin != cout or stride != 1:
            self.branch1_conv = nn.Conv3d(cin, cout, 1, stride=(1, stride, stride), bias=False)
            self.branch1_norm = nn.BatchNorm3d(cout, eps=1e-5, momentum=0.1)
        else:
            self.branch1_conv = None
            self.branch1_norm = None
        self.branch2 = _Branch2(cin, inner, cout, kt, stride)
        self.activation = nn.ReLU()


class _ResStage(nn.Module):
    def __init__(self, cin, inner, cout, kt, stride, depth):
        super().__init__()
        self.res_blocks = nn.ModuleList(
            [_ResBlock(cin if i == 0 else cout, inner, cout, kt, stride if i == 0 else 1) for i in range(depth)])


class _MultiPathway(nn.Module):
    def __init__(self, pathways, fusion):
        super().__init__()
        self.multipathway_blocks = nn.ModuleList(pathways)
        self.multipathway_fusion = fusion


class _PoolConcat(nn.Module):
    def __init__(self, kernel_sizes):
        super().__init__()
        self.pool = nn.ModuleList([nn.AvgPool3d(tuple(k), stride=(1, 1, 1), padding=(0, 0, 0)) for k in kernel_sizes])
        self.dim = 1


class _Head(nn.Module):
    def __init__(self, dim, num_classes, dropout):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.proj = nn.Linear(dim, num_classes)
        self.output_pool = nn.AdaptiveAvgPool3d(1)


class SlowFast(nn.Module):
    """pytorchvideo's `Net` of slowfast_r50: `blocks[0]` stems + fusion, `blocks[1..4]` res stages (+ fusion for 1..3), `blocks[5]`
    pooling + concat, `blocks[6]` head.  `blocks[6].proj` may be replaced by any nn.Linear(2304, k): the head reads it at call time."""

    def __init__(self, head_pool_kernel_sizes=((8, 7, 7), (32, 7, 7)), num_classes=400, dropout_rate=0.5):
        super().__init__()
        blocks = [_MultiPathway([_Stem(STEM_OUT[0], 1), _Stem(STEM_OUT[1], 5)], _Fusion(STEM_OUT[1]))]
        slow_in = STEM_OUT[0] + FUSION_RATIO * STEM_OUT[1]
        fast_in = STEM_OUT[1]
        for s in range(4):
            slow = _ResStage(slow_in, SLOW_INNER[s], SLOW_OUT[s], SLOW_CONV_A_T[s], STAGE_STRIDE[s], DEPTHS[s])
            fast = _ResStage(fast_in, FAST_INNER[s], FAST_OUT[s], FAST_CONV_A_T[s], STAGE_STRIDE[s], DEPTHS[s])
            fusion = _Fusion(FAST_OUT[s]) if s < 3 else None
            blocks.append(_MultiPathway([slow, fast], fusion))
            slow_in = SLOW_OUT[s] + (FUSION_RATIO * FAST_OUT[s] if s < 3 else 0)
            fast_in = FAST_OUT[s]
        blocks.append(_PoolConcat(head_pool_kernel_sizes))
        blocks.append(_Head(HEAD_DIM, num_classes, dropout_rate))
        self.blocks = nn.ModuleList(blocks)
        self.head_pool_kernel_sizes = tuple(tuple(int(v) for v in k) for k in head_pool_kernel_sizes)
        # dropout draws: torch.rand unless set to fn(shape, device) -> uniforms of `shape` (shape = the pooled [B, 2304, Pt, Ph, Pw])
        self.dropout_uniform = None
        self.reset_parameters()

    def reset_parameters(self):
        """pytorchvideo's init_net_weights(style="resnet"): convolutions c2_msra_fill, BatchNorm weight 1 (0 for the last one of every
        bottleneck), bias 0; the projection normal(0, 0.01) with zero bias."""
        for m in self.modules():
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm3d):
                nn.init.constant_(m.weight, 0.0 if getattr(m, "block_final_bn", False) else 1.0)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.01)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Accepts pytorchvideo checkpoints, also as saved from an nn.DataParallel wrap (`module.` prefix)."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

    def forward(self, x):
        from . import slowfast_engine
        return slowfast_engine.slowfast_apply(self, x)


def slowfast_r50(pretrained=False, weights_path=None, head_pool_kernel_sizes=((8, 7, 7), (32, 7, 7)), **kwargs):
    """torch.hub entry point with pytorchvideo's signature.  `pretrained=True` needs a local `weights_path` (a pytorchvideo state dict,
    e.g. SLOWFAST_8x8_R50.pyth's "model_state"): the Kinetics checkpoint is not fetched from the network."""
    model = SlowFast(head_pool_kernel_sizes=head_pool_kernel_sizes, **kwargs)
    if pretrained and weights_path is None:
        raise RuntimeError("slowfast_r50(pretrained=True) downloads the Kinetics-400 checkpoint, which needs network access; pass "
                           "weights_path=<local pytorchvideo state dict> instead")
    if weights_path is not None:
        sd = torch.load(weights_path, map_location="cpu")
        if isinstance(sd, dict) and "model_state" in sd:
            sd = sd["model_state"]
        model.load_state_dict(sd)
    return model


# ---- input transform (reference utils.py:140-186) -------------------------------------------------------------------------------

def frame_indices(n_in, n_out):
    """`torch.linspace(0, n_in - 1, n_out).long()` (UniformTemporalSubsample, PackPathway) in integer arithmetic."""
    if n_out == 1:
        return [0]
    return [(i * (n_in - 1)) // (n_out - 1) for i in range(n_out)]


def frame_sources(fidx, F):
    """The inverse of a frame selection, CSR style: (start, j) with j[start[f]:start[f + 1]] = the output frames that selected source
    frame f, ascending (the summation order of mt_sf_ingest_bwd); a frame nobody selected has an empty range."""
    fidx = [int(f) for f in fidx]
    if fidx and not 0 <= min(fidx) <= max(fidx) < F:
        raise ValueError(f"frame index out of range for {F} frames")
    start = [0] * (F + 1)
    for f in fidx:
        start[f + 1] += 1
    for f in range(F):
        start[f + 1] += start[f]
    fill = list(start[:F])
    js = [0] * len(fidx)
    for j, f in enumerate(fidx):
        js[fill[f]] = j
        fill[f] += 1
    return start, js


def _packed_view(buf):
    """[B, T, H, W, 4] packed buffer -> the [B, 3, T, H, W] tensor the reference's transform returns (a view, no copy)."""
    v = buf[..., :3].permute(0, 4, 1, 2, 3)
    v._mt_packed = buf
    return v


def ingest(src, fidx, normalize, layout, split=None):
    """One mt_sf_ingest launch: frames fidx of src (uint8 or fp32; layout 'bfhwc' or 'bcfhw') -> packed [B, T, H, W, 4] buffers: one
    of len(fidx) frames, or two (the first `split` frames, then the rest) when split is given."""
    if layout == "bfhwc":
        B, F, H, W, _ = src.shape
        sb, sf, sh, sw, sc = src.stride()
    else:
        B, _, F, H, W = src.shape
        sb, sc, sf, sh, sw = src.stride()
    if max(fidx) >= F:
        raise ValueError(f"frame index {max(fidx)} out of range for {F} frames")
    is_u8 = src.dtype == torch.uint8
    if not is_u8 and src.dtype != torch.float32:
        src = src.float()
        sb, sf, sh, sw, sc = [src.stride(i) for i in ((0, 1, 2, 3, 4) if layout == "bfhwc" else (0, 2, 3, 4, 1))]
    n = len(fidx)
    split = n if split is None else split
    out = torch.empty(B, split, H, W, 4, dtype=torch.float32, device=src.device)
    out2 = torch.empty(B, n - split, H, W, 4, dtype=torch.float32, device=src.device) if split < n else None
    idx = torch.tensor(fidx, dtype=torch.int32).to(src.device)
    L.mt.sf_ingest(src, int(is_u8), sb, sf, sh, sw, sc, idx, n, split, B, H, W, int(normalize), out, out2)
    return out if out2 is None else (out, out2)


def _src_strides(src, layout):
    """Element strides (b, f, h, w, c) of a clip tensor in either layout."""
    return [src.stride(i) for i in ((0, 1, 2, 3, 4) if layout == "bfhwc" else (0, 2, 3, 4, 1))]


_SOURCES = {}


def _sources_on_device(fidx, F, device):
    """frame_sources(fidx, F) as int32 device tensors, kept per selection (a training loop asks for the same one every step)."""
    key = (fidx, F, str(device))
    hit = _SOURCES.get(key)
    if hit is None:
        if len(_SOURCES) >= 64:
            _SOURCES.clear()
        start, js = frame_sources(list(fidx), F)
        hit = _SOURCES[key] = (torch.tensor(start, dtype=torch.int32).to(device), torch.tensor(js, dtype=torch.int32).to(device))
    return hit


def ingest_bwd(dout, dout2, fidx, shape, normalize, layout, split=None):
    """One mt_sf_ingest_bwd launch, the adjoint of ingest(): gradients of the packed buffers ([B, T, H, W, 4]; dout2 None without a
    split) -> the fp32 gradient of the source clip of `shape` in `layout`."""
    if layout == "bfhwc":
        B, F, H, W, _ = shape
    else:
        B, _, F, H, W = shape
    n = len(fidx)
    split = n if split is None else split
    want = [(B, split, H, W, 4)] + ([(B, n - split, H, W, 4)] if split < n else [])
    got = [tuple(d.shape) for d in (dout, dout2) if d is not None]
    if got != want:
        raise ValueError(f"ingest_bwd: packed gradients of shapes {got}, expected {want}")
    dout = dout.contiguous().float()
    dout2 = dout2.contiguous().float() if dout2 is not None else None
    dsrc = torch.empty(tuple(shape), dtype=torch.float32, device=dout.device)
    st, jl = _sources_on_device(tuple(fidx), F, dout.device)
    sb, sf, sh, sw, sc = _src_strides(dsrc, layout)
    L.mt.sf_ingest_bwd(dout, dout2, st, jl, F, n, split, B, H, W, int(normalize), dsrc, sb, sf, sh, sw, sc)
    return dsrc


class _Ingest(torch.autograd.Function):
    """ingest() of an fp32 clip that requires grad; the backward is mt_sf_ingest_bwd."""

    @staticmethod
    def forward(ctx, src, fidx, normalize, layout, split):
        ctx.meta = (tuple(fidx), tuple(src.shape), bool(normalize), layout, split)
        out = ingest(src, fidx, normalize, layout, split)
        return out if isinstance(out, tuple) else (out,)

    @staticmethod
    def backward(ctx, *g):
        fidx, shape, normalize, layout, split = ctx.meta
        n = len(fidx)
        sizes = [n] if split is None or split == n else [split, n - split]
        B, H, W = (shape[0], shape[2], shape[3]) if layout == "bfhwc" else (shape[0], shape[3], shape[4])
        g = [gi if gi is not None else torch.zeros(B, t, H, W, 4, dtype=torch.float32, device=next(x for x in g if x is not None).device)
             for gi, t in zip(g, sizes)]
        return ingest_bwd(g[0], g[1] if len(g) > 1 else None, list(fidx), shape, normalize, layout, split), None, None, None, None


# ---- ShortSideScale + CenterCropVideo (reference utils.py:176-177) ------------------------------------------------------------------
# The size rule is pytorchvideo's short_side_scale and the crop rounding torchvision's center_crop, restated from their published
# source and not checked against either package.  The interpolation itself is checked against F.interpolate.

def resize_geometry(H, W, side_size, crop_size):
    """(Hr, Wr, top, left): the frame size after ShortSideScale(side_size) of H x W frames and the corner of the
    CenterCropVideo(crop_size) window in it.  The short side becomes side_size, the long one floor(long / short * side_size); the
    corner is Python's round((size - crop_size) / 2.0), halves to the even integer."""
    if W < H:
        Hr, Wr = int(math.floor(float(H) / W * side_size)), side_size
    else:
        Hr, Wr = side_size, int(math.floor(float(W) / H * side_size))
    if Hr < crop_size or Wr < crop_size:
        raise ValueError("height and width must be no smaller than crop_size")
    return Hr, Wr, int(round((Hr - crop_size) / 2.0)), int(round((Wr - crop_size) / 2.0))


def axis_taps(n_in, n_out, first=0, count=None, dtype=torch.float32):
    """The two taps of bilinear interpolation (align_corners=False, no antialiasing) along one axis, n_in -> n_out, for the `count`
    output indices from `first` on (default: all): (i0, i1, lam) as CPU tensors (int32, int32, dtype), with
    value[first + d] = (1 - lam[d]) * x[i0[d]] + lam[d] * x[i1[d]].  Computed in `dtype` the way F.interpolate does in that dtype."""
    count = n_out - first if count is None else count
    d = torch.arange(first, first + count, dtype=dtype)
    scale = torch.tensor(float(n_in), dtype=dtype) / n_out
    src = (scale * (d + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    lam = (src - i0.to(dtype)).clamp(0, 1)
    return i0.int(), i1.int(), lam


def axis_sources(i0, i1, lam, n_in):
    """The inverse of axis_taps, CSR style: (start, out, wt) with out[start[s]:start[s + 1]] = the output indices that reference
    source index s and wt their weights (1 - lam as i0, lam as i1), output index ascending, i0 before i1 (the summation order of
    mt_sf_ingest_resize_bwd).  A clamped edge (i1 == i0) lists both weights; a weight of exactly 0 references nothing."""
    w0, w1 = (1 - lam).tolist(), lam.tolist()
    refs = [[] for _ in range(n_in)]
    for d, (a, b) in enumerate(zip(i0.tolist(), i1.tolist())):
        if w0[d] != 0:
            refs[a].append((d, w0[d]))
        if w1[d] != 0:
            refs[b].append((d, w1[d]))
    start = [0]
    for r in refs:
        start.append(start[-1] + len(r))
    return start, [d for r in refs for d, _ in r], [w for r in refs for _, w in r]


_RESIZE_TABLES = {}


def _resize_tables(Hs, Ws, geom, device):
    """Device tables of one geometry (Hr, Wr, top, left, Ho, Wo) of Hs x Ws frames, kept like _sources_on_device: per axis the forward's
    (idx [2][n] int32, lam [n] fp32) and the backward's (start, out, wt), all from one fp32 axis_taps table."""
    key = (Hs, Ws, tuple(geom), str(device))
    hit = _RESIZE_TABLES.get(key)
    if hit is None:
        if len(_RESIZE_TABLES) >= 64:
            _RESIZE_TABLES.clear()
        Hr, Wr, top, left, Ho, Wo = geom
        hit = []
        for n_in, n_out, first, count in ((Hs, Hr, top, Ho), (Ws, Wr, left, Wo)):
            i0, i1, lam = axis_taps(n_in, n_out, first, count)
            start, out, wt = axis_sources(i0, i1, lam, n_in)
            hit += [torch.stack([i0, i1]).to(device), lam.to(device), torch.tensor(start, dtype=torch.int32).to(device),
                    torch.tensor(out, dtype=torch.int32).to(device), torch.tensor(wt, dtype=torch.float32).to(device)]
        hit = _RESIZE_TABLES[key] = tuple(hit)
    return hit


def _dense(shape, strides):
    """True when the strides address every element of one block of prod(shape) elements once: a permutation of a contiguous tensor."""
    expect = 1
    for s, n in sorted((s, n) for n, s in zip(shape, strides) if n != 1):
        if s != expect:
            return False
        expect *= n
    return True


def _check_geometry(geom):
    Hr, Wr, top, left, Ho, Wo = geom
    if Hr < Ho or Wr < Wo:
        raise ValueError("height and width must be no smaller than crop_size")


def ingest_resize(src, fidx, normalize, layout, geom, split=None):
    """One mt_sf_ingest_resize launch: ingest() with the frames resized (bilinear) to geom's Hr x Wr and cropped to its Ho x Wo
    window at (top, left); geom = (Hr, Wr, top, left, Ho, Wo).  Packed [B, T, Ho, Wo, 4] buffers as ingest() returns them."""
    _check_geometry(geom)
    if layout == "bfhwc":
        B, F, H, W, _ = src.shape
    else:
        B, _, F, H, W = src.shape
    if max(fidx) >= F:
        raise ValueError(f"frame index {max(fidx)} out of range for {F} frames")
    is_u8 = src.dtype == torch.uint8
    if not is_u8 and src.dtype != torch.float32:
        src = src.float()
    sb, sf, sh, sw, sc = _src_strides(src, layout)
    Hr, Wr, top, left, Ho, Wo = geom
    n = len(fidx)
    split = n if split is None else split
    out = torch.empty(B, split, Ho, Wo, 4, dtype=torch.float32, device=src.device)
    out2 = torch.empty(B, n - split, Ho, Wo, 4, dtype=torch.float32, device=src.device) if split < n else None
    idx = torch.tensor(fidx, dtype=torch.int32).to(src.device)
    t = _resize_tables(H, W, geom, src.device)
    L.mt.sf_ingest_resize(src, int(is_u8), sb, sf, sh, sw, sc, idx, n, split, B, H, W, t[0], t[1], t[5], t[6], Hr, Wr, top, left, Ho, Wo,
                          int(normalize), out, out2)
    return out if out2 is None else (out, out2)


def ingest_resize_bwd(dout, dout2, fidx, shape, normalize, layout, geom, split=None, strides=None):
    """One mt_sf_ingest_resize_bwd launch, the adjoint of ingest_resize(): gradients of the packed buffers ([B, T, Ho, Wo, 4]) -> the
    fp32 gradient of the source clip of `shape` in `layout`, contiguous or with the given `strides` (those of a dense source, e.g. the
    permuted view of train.py:357: the gradient is then written in the source's own memory order)."""
    _check_geometry(geom)
    if layout == "bfhwc":
        B, F, H, W, _ = shape
    else:
        B, _, F, H, W = shape
    Hr, Wr, top, left, Ho, Wo = geom
    n = len(fidx)
    split = n if split is None else split
    want = [(B, split, Ho, Wo, 4)] + ([(B, n - split, Ho, Wo, 4)] if split < n else [])
    got = [tuple(d.shape) for d in (dout, dout2) if d is not None]
    if got != want:
        raise ValueError(f"ingest_resize_bwd: packed gradients of shapes {got}, expected {want}")
    dout = dout.contiguous().float()
    dout2 = dout2.contiguous().float() if dout2 is not None else None
    if strides is None:
        dsrc = torch.empty(tuple(shape), dtype=torch.float32, device=dout.device)
    else:
        if not _dense(shape, strides):
            raise ValueError(f"ingest_resize_bwd: strides {tuple(strides)} are not those of a dense tensor of shape {tuple(shape)}")
        dsrc = torch.empty_strided(tuple(shape), tuple(strides), dtype=torch.float32, device=dout.device)
    st, jl = _sources_on_device(tuple(fidx), F, dout.device)
    t = _resize_tables(H, W, geom, dout.device)
    sb, sf, sh, sw, sc = _src_strides(dsrc, layout)
    L.mt.sf_ingest_resize_bwd(dout, dout2, st, jl, F, n, split, B, H, W, t[2], t[3], t[4], t[7], t[8], t[9], Hr, Wr, top, left, Ho, Wo,
                              int(normalize), dsrc, sb, sf, sh, sw, sc)
    return dsrc


class _IngestResize(torch.autograd.Function):
    """ingest_resize() of an fp32 clip that requires grad; the backward is mt_sf_ingest_resize_bwd."""

    @staticmethod
    def forward(ctx, src, fidx, normalize, layout, geom, split):
        strides = tuple(src.stride()) if _dense(src.shape, src.stride()) else None          # the gradient follows a dense source's layout
        ctx.meta = (tuple(fidx), tuple(src.shape), bool(normalize), layout, tuple(geom), split, strides)
        out = ingest_resize(src, fidx, normalize, layout, geom, split)
        return out if isinstance(out, tuple) else (out,)

    @staticmethod
    def backward(ctx, *g):
        fidx, shape, normalize, layout, geom, split, strides = ctx.meta
        n = len(fidx)
        sizes = [n] if split is None or split == n else [split, n - split]
        device = next(x for x in g if x is not None).device
        g = [gi if gi is not None else torch.zeros(shape[0], t, geom[4], geom[5], 4, dtype=torch.float32, device=device)
             for gi, t in zip(g, sizes)]
        return (ingest_resize_bwd(g[0], g[1] if len(g) > 1 else None, list(fidx), shape, normalize, layout, geom, split, strides),
                None, None, None, None, None)


def _wants_grad(x):
    return torch.is_grad_enabled() and x.is_floating_point() and x.requires_grad


INTERPOLATIONS = ("bilinear",)


def slowfast_input_transform(videos, crop_size=256, side_size=256, num_frames=NUM_FRAMES, device=None, interpolation=None):
    """utils.py:166-186 for a batch: `videos` [B, F, H, W, 3] (the loader's layout) or [B, 3, F, H, W] (after train.py:357's
    rearrange; the permuted view is read in place), uint8 or fp32, contiguous or strided.  Returns [slow [B, 3, 8, crop, crop],
    fast [B, 3, 32, crop, crop]] on the device, as train.py:358 builds them: UniformTemporalSubsample(32), /255, Normalize(0.45, 0.225),
    ShortSideScale(side_size), CenterCropVideo(crop_size), PackPathway -- one launch.

    interpolation=None (default): the two spatial steps are only accepted where they are identities, side_size x side_size frames with
    crop_size == side_size (the configured 256 x 256 of config/slowfast.yaml); anything else raises NotImplementedError.
    interpolation="bilinear" (the name is pytorchvideo's ShortSideScale(interpolation=...) argument): frames of any size.  The short
    side is scaled to side_size with F.interpolate(mode="bilinear", align_corners=False) arithmetic, no antialiasing, every tap
    normalised before it is interpolated (the reference's order); the crop window's corner is resize_geometry()'s.  A crop larger
    than the resized frame raises ValueError, as torchvision does.  Frames that need neither step take the same launch, and give the
    same bits, as interpolation=None.  fp32 videos that require grad get their gradient through either path (uint8 has none)."""
    if not torch.is_tensor(videos) or videos.dim() != 5:
        raise ValueError("slowfast_input_transform: expected a [B, F, H, W, 3] or [B, 3, F, H, W] tensor")
    if interpolation is not None and interpolation not in INTERPOLATIONS:
        raise NotImplementedError(f"slowfast_input_transform: interpolation={interpolation!r} is not implemented; the supported mode is "
                                  "'bilinear' (align_corners=False, no antialiasing)")
    layout = "bfhwc" if videos.shape[-1] == 3 else "bcfhw"
    if layout == "bcfhw" and videos.shape[1] != 3:
        raise ValueError(f"slowfast_input_transform: no 3-channel axis in {tuple(videos.shape)}")
    H, W = (videos.shape[2], videos.shape[3]) if layout == "bfhwc" else (videos.shape[3], videos.shape[4])
    geom = None
    if not (H == W == crop_size == side_size):
        if interpolation is None:
            raise NotImplementedError(f"slowfast_input_transform: ShortSideScale({side_size}) + CenterCrop({crop_size}) are only the "
                                      f"identity for {side_size} x {side_size} frames (config/slowfast.yaml); got {H} x {W} -- pass "
                                      "interpolation='bilinear' for the resize")
        geom = resize_geometry(H, W, side_size, crop_size) + (crop_size, crop_size)
    if not videos.is_cuda:
        videos = videos.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    F = videos.shape[1] if layout == "bfhwc" else videos.shape[2]
    fi = frame_indices(F, num_frames)
    si = frame_indices(num_frames, num_frames // ALPHA)
    sel = [fi[j] for j in si] + fi
    grad = _wants_grad(videos)          # fp32 videos that require grad: the packing is part of the graph (uint8 has no gradient)
    if geom is None:
        slow, fast = _Ingest.apply(videos.float(), sel, True, layout, len(si)) if grad else ingest(videos, sel, True, layout, split=len(si))
    elif grad:
        slow, fast = _IngestResize.apply(videos.float(), sel, True, layout, geom, len(si))
    else:
        slow, fast = ingest_resize(videos, sel, True, layout, geom, split=len(si))
    return [_packed_view(slow), _packed_view(fast)]


def pack_pathway_input(x):
    """A pathway input [B, 3, T, H, W] -> packed [B, T, H, W, 4] (no copy when it came from slowfast_input_transform)."""
    buf = getattr(x, "_mt_packed", None)
    # the transform's buffer serves as it is unless a gradient is asked of a view whose buffer has no history (requires_grad_() on the
    # transform's outputs of uint8 videos, or of a no_grad transform): that view is then packed again, inside the graph
    if buf is not None and buf.is_cuda and (buf.requires_grad or not _wants_grad(x)):
        return buf
    if not x.is_cuda:
        raise L.MintimeHipError("SlowFast (MI355X build) needs device tensors; there is no CPU path")
    if x.dim() != 5 or x.shape[1] != 3:
        raise ValueError(f"expected a [B, 3, T, H, W] pathway input, got {tuple(x.shape)}")
    if _wants_grad(x):
        return _Ingest.apply(x.float(), list(range(x.shape[2])), False, "bcfhw", None)[0]
    return ingest(x.detach(), list(range(x.shape[2])), False, "bcfhw")


__all__ = ["SlowFast", "slowfast_r50", "slowfast_input_transform", "frame_indices", "frame_sources", "resize_geometry", "axis_taps",
           "axis_sources"]
