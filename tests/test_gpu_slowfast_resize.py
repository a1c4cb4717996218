"""SlowFast's input transform with ShortSideScale + CenterCropVideo on the device (interpolation="bilinear": mt_sf_ingest_resize and its
adjoint mt_sf_ingest_resize_bwd) against the reference chain in fp64 torch on the CPU (tests/sf_resize_ref.py).

Gates are ratios: the device's error against fp64 over the error of torch's own fp32 CPU run of the same chain on the same input (the
arithmetic is the same fp32 lerp, so the ratio is of order 1).  Each gate is twice the worst ratio measured on an MI355X, rounded up
(the convention of test_gpu_slowfast_input_grad.py); the measured value stands beside the constant and both errors are printed."""
import functools

import pytest
import torch
import torch.nn.functional as F

import mintime_amd
from mintime_amd import harness, optim, lib as L, slowfast as S

from . import sf_resize_ref as RR
from . import slowfast_ref as R
from . import test_gpu_slowfast as TS
from . import test_gpu_slowfast_input_grad as IG
from .test_slowfast_resize_host import GEOMETRY, IDS

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
NAN = float("nan")
GUARD = 64                      # floats of NaN guard band on each side of a packed buffer (keeps the 16-byte alignment)
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
B = 2
FRAMES = [5, 40]                # 5 repeats frames, 40 skips some
# downscaling and scale-1 rows: no sample lands on a source pixel centre except at scale 1, where all do, so fp32 and fp64 pick the
# same taps and the gradient's support can be compared exactly (upscaling may split a sample differently at weights near 0 and 1)
SUPPORT_ROWS = {(20, 28), (28, 20), (16, 21), (16, 23), (37, 53)}

# measured worst ratios to torch-fp32's own error (MI355X), each gate twice that, rounded up
FWD_T32_FACTOR = 2.2            # 1.06 ((13, 9, 16, 12), F = 5: 2.13e-6 against 2.01e-6); every other case 0.93 .. 1.01
ADJ_T32_FACTOR = 4.3            # 2.12 ((13, 9, 16, 12), F = 5: 4.22e-7 against 1.99e-7); next (9, 13, 16, 16), F = 5: 1.50; others <= 1.23
NET_T32_FACTOR = 2.1            # 1.00 in both layouts (relative L2 4.62e-3 against torch-fp32's 4.60e-3)


def _selection(Fr):
    fi = S.frame_indices(Fr, 32)
    si = S.frame_indices(32, 8)
    return [fi[j] for j in si] + fi


def _geom(case):
    H, W, side, crop = case
    return S.resize_geometry(H, W, side, crop) + (crop, crop)


def _maxabs(got, ref):
    return max((a.detach().cpu().double() - b.detach().double()).abs().max().item() for a, b in zip(got, ref))


@functools.lru_cache(maxsize=None)
def _forward_case(i, Fr):
    """The uint8 clip of geometry row i with Fr frames and the reference pathways in fp64 and fp32 (shared, never modified)."""
    H, W, side, crop = GEOMETRY[i][0]
    g = torch.Generator().manual_seed(100 * i + Fr)
    v = torch.randint(0, 256, (B, Fr, H, W, 3), generator=g, dtype=torch.uint8)
    with torch.no_grad():
        return v, RR.transform(v, "bfhwc", torch.float64, crop, side), RR.transform(v, "bfhwc", torch.float32, crop, side)


def _raw_forward(src, layout, sel, geom, out, out2):
    Bn, Fr, H, W = (src.shape[0], src.shape[1], src.shape[2], src.shape[3]) if layout == "bfhwc" else \
        (src.shape[0], src.shape[2], src.shape[3], src.shape[4])
    t = S._resize_tables(H, W, geom, dev)
    idx = torch.tensor(sel, dtype=torch.int32).to(dev)
    rc = L.get().mt_sf_ingest_resize(L.ptr(src), int(src.dtype == torch.uint8), *S._src_strides(src, layout), L.ptr(idx), len(sel), 8, Bn, H,
                                     W, L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[5]), L.ptr(t[6]), *geom, 1, L.ptr(out), L.ptr(out2),
                                     L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _guarded(n):
    buf = torch.full((GUARD + n + GUARD,), NAN, device=dev)
    return buf, buf[GUARD:GUARD + n]


# ---- 1. forward --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Fr", FRAMES)
@pytest.mark.parametrize("i", range(len(GEOMETRY)), ids=IDS)
def test_forward_against_fp64(i, Fr):
    case = GEOMETRY[i][0]
    crop = case[3]
    v, ref64, ref32 = _forward_case(i, Fr)
    e32 = _maxabs(ref32, ref64)
    first = None
    for dtype in (torch.uint8, torch.float32):
        for layout in ("bfhwc", "bcfhw"):
            src = v.to(dtype).to(dev)
            if layout == "bcfhw":
                src = src.permute(0, 4, 1, 2, 3)                              # train.py:357's view, not a copy
                assert not src.is_contiguous()
            slow, fast = mintime_amd.slowfast_input_transform(src, crop_size=crop, side_size=case[2], interpolation="bilinear")
            torch.cuda.synchronize()
            assert slow.shape == (B, 3, 8, crop, crop) and fast.shape == (B, 3, 32, crop, crop) and slow.dtype == torch.float32
            assert slow._mt_packed.shape == (B, 8, crop, crop, 4) and fast._mt_packed.shape == (B, 32, crop, crop, 4)
            assert slow._mt_packed.data_ptr() == slow.data_ptr()                 # views of the packed buffers
            assert not bool(slow._mt_packed[..., 3].any()) and not bool(fast._mt_packed[..., 3].any())      # the 4th channel is 0
            e = _maxabs([slow, fast], ref64)
            print(f"resize forward {case} F={Fr} {str(dtype)[6:]} {layout}: max abs err {e:.2e} (torch fp32 {e32:.2e}, ratio {e / e32:.2f})")
            assert e <= FWD_T32_FACTOR * e32, (e, e32)
            got = (slow._mt_packed.cpu(), fast._mt_packed.cpu())
            if first is None:
                first = got
            # uint8 and fp32 sources of the same values, in either layout, and a second launch: the same bits
            assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
    # the raw entry point into guarded buffers: the same bits again, and nothing outside the buffers is written
    n0, n1 = B * 8 * crop * crop * 4, B * 32 * crop * crop * 4
    (b0, o0), (b1, o1) = _guarded(n0), _guarded(n1)
    L.check(_raw_forward(v.to(dev), "bfhwc", _selection(Fr), _geom(case), o0, o1), "mt_sf_ingest_resize")
    for buf, n, want in ((b0.cpu(), n0, first[0]), (b1.cpu(), n1, first[1])):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all()
        assert torch.equal(buf[GUARD:GUARD + n].reshape(want.shape), want)


# ---- 2. nothing to resample --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Fr", FRAMES)
def test_no_resample_is_the_plain_ingest(Fr):
    g = torch.Generator().manual_seed(7 + Fr)
    v = torch.randint(0, 256, (B, Fr, 16, 16, 3), generator=g, dtype=torch.uint8).to(dev)
    for src in (v, v.permute(0, 4, 1, 2, 3), v.float()):
        a = mintime_amd.slowfast_input_transform(src, crop_size=16, side_size=16)
        b = mintime_amd.slowfast_input_transform(src, crop_size=16, side_size=16, interpolation="bilinear")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0]._mt_packed, b[0]._mt_packed) and torch.equal(a[1]._mt_packed, b[1]._mt_packed)


# ---- 3. the adjoint ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _adjoint_case(i, Fr):
    """fp32 clip, positive packed gradients, and the clip gradient of the reference chain in fp64 and fp32 ([B, F, H, W, 3])."""
    H, W, side, crop = GEOMETRY[i][0]
    g = torch.Generator().manual_seed(200 * i + Fr)
    v = torch.rand(B, Fr, H, W, 3, generator=g) * 255
    douts = [torch.rand(B, t, crop, crop, 4, generator=g) + 0.5 for t in (8, 32)]
    for d in douts:
        d[..., 3] = NAN                                                          # must not reach dsrc

    def grad(dt):
        x = v.to(dt).clone().requires_grad_(True)
        slow, fast = RR.transform(x, "bfhwc", dt, crop, side)
        loss = sum((p * d[..., :3].permute(0, 4, 1, 2, 3).to(dt)).sum() for p, d in zip((slow, fast), douts))
        loss.backward()
        return x.grad
    return v, douts, grad(torch.float64), grad(torch.float32)


@pytest.mark.parametrize("Fr", FRAMES)
@pytest.mark.parametrize("i", range(len(GEOMETRY)), ids=IDS)
def test_adjoint_against_fp64_autograd(i, Fr):
    case = GEOMETRY[i][0]
    H, W = case[:2]
    v, douts, ref64, ref32 = _adjoint_case(i, Fr)
    sel, geom = _selection(Fr), _geom(case)
    d0, d1 = [d.to(dev) for d in douts]
    e32 = _maxabs([ref32], [ref64])
    got = {}
    view = v.permute(0, 4, 1, 2, 3)                                              # train.py:357's view: bcfhw shape, bfhwc memory
    for name, layout, shape, strides in (("bfhwc", "bfhwc", (B, Fr, H, W, 3), None), ("bcfhw", "bcfhw", (B, 3, Fr, H, W), None),
                                         ("view", "bcfhw", (B, 3, Fr, H, W), view.stride())):
        a = S.ingest_resize_bwd(d0, d1, sel, shape, True, layout, geom, split=8, strides=strides)
        b = S.ingest_resize_bwd(d0, d1, sel, shape, True, layout, geom, split=8, strides=strides)
        torch.cuda.synchronize()
        assert a.shape == shape and a.dtype == torch.float32
        assert a.stride() == (view.stride() if strides else torch.empty(shape).stride())      # the source's shape, strides and layout
        assert torch.equal(a, b)                                                 # the same bits from launch to launch
        got[name] = a.cpu()
    g = got["bfhwc"]
    assert torch.equal(got["bcfhw"].permute(0, 2, 3, 4, 1), g) and torch.equal(got["view"].permute(0, 2, 3, 4, 1), g)      # one sum
    assert bool(torch.isfinite(g).all())
    e = _maxabs([g], [ref64])
    print(f"resize adjoint {case} F={Fr}: max abs err {e:.2e} (torch fp32 {e32:.2e}, ratio {e / e32:.2f})")
    assert e <= ADJ_T32_FACTOR * e32, (e, e32)
    unselected = [f for f in range(Fr) if f not in sel]
    assert (len(unselected) > 0) == (Fr == 40)
    assert not bool(g[:, unselected].any())                                      # frames nobody selected: exact 0
    if (H, W) in SUPPORT_ROWS:
        assert torch.equal(g == 0, ref64 == 0)                                   # the support is the crop's footprint, exactly
        assert bool((ref64[:, sel[0]] == 0).any())                               # ... and the crop does leave pixels out
    # through autograd from the permuted view of a [B, F, H, W, 3] leaf: the gradient arrives in the leaf's shape with the same bits
    leaf = v.to(dev).requires_grad_(True)
    slow, fast = mintime_amd.slowfast_input_transform(leaf.permute(0, 4, 1, 2, 3), crop_size=case[3], side_size=case[2],
                                                      interpolation="bilinear")
    clean = [torch.nan_to_num(d[..., :3], nan=0.0).permute(0, 4, 1, 2, 3) for d in (d0, d1)]
    torch.autograd.backward([slow, fast], clean)
    torch.cuda.synchronize()
    assert leaf.grad.shape == v.shape and leaf.grad.stride() == leaf.stride() and leaf.grad.dtype == torch.float32
    assert torch.equal(leaf.grad.cpu(), g)


def test_offsets_past_2_31_elements():
    """Every offset is 64-bit: a packed buffer, a source clip batch and a clip gradient of more than 2^31 elements each.  The far end
    of each is compared, on the device, with the same work done at offset 0 (a wrapped offset would land elsewhere)."""
    g = torch.Generator(device=dev).manual_seed(5)
    # packed output: 33 fast frames of 4096 x 4096 x 4 floats = 2.2e9; every output frame selects source frame 0, so all are equal
    src = torch.randint(0, 256, (1, 1, 8, 8, 3), device=dev, generator=g, dtype=torch.uint8)
    slow, fast = S.ingest_resize(src, [0] * 34, True, "bfhwc", S.resize_geometry(8, 8, 4096, 4096) + (4096, 4096), split=1)
    assert fast.numel() > 2 ** 31
    assert torch.equal(fast[0, 32], slow[0, 0]) and torch.equal(fast[0, 0], slow[0, 0]) and bool(torch.isfinite(slow).all())
    del slow, fast
    # source: 4 uint8 clips of 16384 x 16384 x 3 = 3.2e9 elements; the last clip alone gives the same bits
    src = torch.randint(0, 256, (4, 1, 16384, 16384, 3), device=dev, generator=g, dtype=torch.uint8)
    assert src.numel() > 2 ** 31 and 3 * src.stride(0) > 2 ** 31
    geom = S.resize_geometry(16384, 16384, 16, 16) + (16, 16)
    whole = S.ingest_resize(src, [0] * 40, True, "bfhwc", geom, split=8)
    last = S.ingest_resize(src[3:], [0] * 40, True, "bfhwc", geom, split=8)
    assert all(torch.equal(w[3:], x) for w, x in zip(whole, last)) and float(last[1][..., :3].std()) > 0
    del src, whole, last
    # clip gradient: 11 fp32 clips of 8192 x 8192 x 3 = 2.2e9 elements; the last clip's gradient alone gives the same bits
    d0, d1 = [torch.rand(11, t, 16, 16, 4, device=dev, generator=g) + 0.5 for t in (8, 32)]
    geom = S.resize_geometry(8192, 8192, 16, 16) + (16, 16)
    whole = S.ingest_resize_bwd(d0, d1, [0] * 40, (11, 1, 8192, 8192, 3), True, "bfhwc", geom, split=8)
    last = S.ingest_resize_bwd(d0[10:], d1[10:], [0] * 40, (1, 1, 8192, 8192, 3), True, "bfhwc", geom, split=8)
    assert whole.numel() > 2 ** 31
    assert torch.equal(whole[10:], last) and int((last != 0).sum()) == 32 * 32 * 3      # two taps per axis of each of the 16 x 16 samples
    torch.cuda.synchronize()


# ---- 4. through the network --------------------------------------------------------------------------------------------------------

NET_KW = dict(crop_size=64, side_size=64, interpolation="bilinear")


@pytest.mark.parametrize("layout", ["bfhwc", "bcfhw"])
def test_gradient_through_the_resizing_transform(layout):
    """48 x 80 frames -> (64, 106), crop left = 21; F = 8: every frame is selected 4 times by the fast pathway and once by the slow."""
    assert S.resize_geometry(48, 80, 64, 64) == (64, 106, 0, 21)
    m, ref = IG._eval_model(IG.TRANSFORM_HEAD)
    g = torch.Generator().manual_seed(300)
    videos = torch.randint(0, 256, (2, 8, 48, 80, 3), generator=g).float()
    if layout == "bcfhw":
        videos = videos.permute(0, 4, 1, 2, 3).contiguous()

    def ref_grad(dt, labels):
        sd = {k: (v.to(dt).clone() if v.is_floating_point() else v.clone()) for k, v in ref.items()}
        v = videos.to(dt).clone().requires_grad_(True)
        slow, fast = RR.transform(v, layout, dt, 64, 64)
        y = R.forward(sd, slow, fast, training=False, head_pool_kernel_sizes=IG.TRANSFORM_HEAD)
        labels = IG._live_labels(y) if labels is None else labels
        F.binary_cross_entropy_with_logits(y, labels.to(dt).reshape(-1, 1)).backward()
        return y.detach(), v.grad, labels

    yr, gr, labels = ref_grad(torch.float64, None)
    y32, g32, _ = ref_grad(torch.float32, labels)
    assert all(float(gr[b].abs().max()) > 0 for b in range(2))
    m.zero_grad(set_to_none=True)
    v = videos.to(dev).requires_grad_(True)
    y = m(S.slowfast_input_transform(v, **NET_KW))
    loss = optim.bce_with_logits(y, labels.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert v.grad is not None and v.grad.shape == videos.shape and v.grad.dtype == torch.float32
    e, e32 = IG._l2(v.grad, gr), IG._l2(g32, gr)
    print(f"through the resizing transform {layout}: relative L2 of videos.grad {e:.2e} (torch fp32 {e32:.2e}, ratio {e / e32:.2f})")
    assert e <= NET_T32_FACTOR * e32, (e, e32)
    m.zero_grad(set_to_none=True)
    logits, loss2, dv = harness.slowfast_input_gradient(m, videos.to(dev), labels.to(dev), **NET_KW)
    assert torch.equal(dv, v.grad) and torch.equal(logits, y.detach()) and torch.equal(loss2, loss.detach())
    assert all(p.grad is None for p in m.parameters())                     # torch.autograd.grad leaves every .grad alone
    with pytest.raises(NotImplementedError):                                # the default keeps refusing
        harness.slowfast_input_gradient(m, videos.to(dev), labels.to(dev), crop_size=64, side_size=64)


def test_train_and_eval_steps_take_uint8_clips_of_another_size():
    m, _ = TS._model(seed=310, head=IG.TRANSFORM_HEAD)
    m.train()
    opt = optim.FusedSGD(m.parameters(), lr=0.001, weight_decay=0.0001)
    g = torch.Generator().manual_seed(311)
    videos = torch.randint(0, 256, (2, 8, 48, 80, 3), generator=g, dtype=torch.uint8).to(dev)
    loss = harness.slowfast_train_step(m, opt, videos, torch.tensor([0.0, 1.0], device=dev), **NET_KW)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.requires_grad)
    m.eval()
    y = harness.slowfast_eval_step(m, videos, **NET_KW)
    assert y.shape == (2, 1) and bool(torch.isfinite(y).all())
    with pytest.raises(NotImplementedError):
        harness.slowfast_eval_step(m, videos)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------

def test_crop_larger_than_the_resized_frame_launches_nothing():
    v = torch.zeros(1, 8, 20, 28, 3, dtype=torch.uint8, device=dev)
    plan = L.Plan()
    with pytest.raises(ValueError, match="no smaller than crop_size"):
        with plan:                                                              # a recording plan counts every launch made
            mintime_amd.slowfast_input_transform(v, crop_size=17, side_size=16, interpolation="bilinear")
    assert plan.ops == 0
    with pytest.raises(ValueError, match="no smaller than crop_size"):
        harness.slowfast_input_gradient(None, v.float(), torch.zeros(1, device=dev), crop_size=17, side_size=16, interpolation="bilinear")


def test_raw_entry_points_refuse_before_launching():
    case = GEOMETRY[0][0]
    H, W, _, crop = case
    geom, sel = _geom(case), _selection(5)
    src = torch.zeros(1, 5, H, W, 3, dtype=torch.uint8, device=dev)
    n0, n1 = 8 * crop * crop * 4, 32 * crop * crop * 4
    b0 = torch.full((n0 + 4,), NAN, device=dev)
    b1 = torch.full((n1 + 4,), NAN, device=dev)
    # a packed buffer 4 bytes off a 16-byte boundary
    assert _raw_forward(src, "bfhwc", sel, geom, b0[1:1 + n0], b1[:n1]) == MT_ERR_UNSUPPORTED
    assert b"mt_sf_ingest_resize" in L.get().mt_last_error()
    assert _raw_forward(src, "bfhwc", sel, geom, b0[:n0], b1[1:1 + n1]) == MT_ERR_UNSUPPORTED
    # a crop window that leaves the resized frame
    Hr, Wr, top, left, Ho, Wo = geom
    assert _raw_forward(src, "bfhwc", sel, (Hr, Wr, top, Wr - Wo + 1, Ho, Wo), b0[:n0], b1[:n1]) == MT_ERR_ARG
    assert _raw_forward(src, "bfhwc", sel, (Hr, Wr, -1, left, Ho, Wo), b0[:n0], b1[:n1]) == MT_ERR_ARG
    assert torch.isnan(b0).all() and torch.isnan(b1).all()                      # nothing was launched
    # the adjoint: misaligned dout, and the same window check; dsrc keeps its fill
    t = S._resize_tables(H, W, geom, dev)
    st, jl = S._sources_on_device(tuple(sel), 5, dev)
    dsrc = torch.full((1, 5, H, W, 3), NAN, device=dev)
    d0, d1 = torch.ones(n0 + 4, device=dev), torch.ones(n1 + 4, device=dev)

    def bwd(p0, p1, gm):
        rc = L.get().mt_sf_ingest_resize_bwd(L.ptr(p0), L.ptr(p1), L.ptr(st), L.ptr(jl), 5, 40, 8, 1, H, W, L.ptr(t[2]), L.ptr(t[3]),
                                             L.ptr(t[4]), L.ptr(t[7]), L.ptr(t[8]), L.ptr(t[9]), *gm, 1, L.ptr(dsrc),
                                             *S._src_strides(dsrc, "bfhwc"), L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert bwd(d0[1:1 + n0], d1[:n1], geom) == MT_ERR_UNSUPPORTED
    assert b"mt_sf_ingest_resize_bwd" in L.get().mt_last_error()
    assert bwd(d0[:n0], d1[1:1 + n1], geom) == MT_ERR_UNSUPPORTED
    assert bwd(d0[:n0], d1[:n1], (Hr, Wr, Hr - Ho + 1, left, Ho, Wo)) == MT_ERR_ARG
    assert torch.isnan(dsrc).all()
    assert bwd(d0[:n0], d1[:n1], geom) == 0 and bool(torch.isfinite(dsrc).all())   # and the well-formed call writes all of dsrc
