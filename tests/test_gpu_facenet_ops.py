"""Per-kernel tests of csrc/facenet.hip against fp64 (torch on the CPU).

mt_conv2d_fwd's bound is derived, not measured: an fp32 MFMA result is a chain of fmaf with one rounding per product, and any
ordering of n such terms errs by at most gamma_n * sum |a_i b_i|; the epilogue adds the bias, the residual scale, the residual sum
(4 more roundings).  Per element, with res = 0 and res_scale = 1 when res is NULL:
    |y - y64| <= 1.01 * (kh kw C + 4) * 2^-24 * (|res| + |res_scale| * (sum |x w| + |bias|))
The shapes are the smallest that can still go wrong: partial row tiles, a reduction that is no multiple of the K step, K that is no
multiple of the column tile, kernels wider than the image, taps that are all padding, channel slices of a wider buffer."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from mintime_amd import lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -12345.5


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv2d(x_rows, N, H, W, Cc, ldx, w, bias, res, ldr, y, ldy, k, s, p, act, scale, grid=None):
    """Launch mt_conv2d_fwd on device row buffers; returns the return code."""
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(s), _pair(p)
    d = L.Conv2dDesc()
    d.N, d.H, d.W, d.C, d.K = N, H, W, Cc, w.shape[0]
    d.Ho, d.Wo = grid if grid else ((H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1)
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.act, d.res_scale = kh, kw, sh, sw, ph, pw, act, scale
    d.ldx, d.ldy, d.ldr = ldx, ldy, ldr
    return L.get().mt_conv2d_fwd(C.byref(d), L.ptr(x_rows), L.ptr(w), L.ptr(bias), L.ptr(res), L.ptr(y), L.stream_ptr())


def run_case(N, H, W, Cc, K, k=1, s=1, p=0, bias=False, res=False, scale=1.0, act=1, yoff=0, ldy=None, xoff=0, ldx=None, seed=0):
    """Runs one layer on the device and returns (y rows [M, K], y64 rows, bound rows, the whole output buffer)."""
    g = torch.Generator().manual_seed(seed)
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(s), _pair(p)
    ldx, ldy = ldx or Cc, ldy or K
    x = torch.randn(N, H, W, Cc, generator=g)
    w = torch.randn(K, kh, kw, Cc, generator=g) * (2.0 / (kh * kw * Cc)) ** 0.5
    b = torch.randn(K, generator=g) * 0.5 if bias else None
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    M = N * Ho * Wo
    ldr = K + 4
    r = torch.randn(M, ldr, generator=g) if res else None
    xbuf = torch.full((N * H * W, ldx), 7.0)
    xbuf[:, xoff:xoff + Cc] = x.reshape(-1, Cc)
    ybuf = torch.full((M, ldy), SENTINEL).cuda()
    xd = xbuf.cuda()
    rc = conv2d(xd.reshape(-1)[xoff:], N, H, W, Cc, ldx, w.cuda(), None if b is None else b.cuda(), None if r is None else r.cuda(), ldr if res else 0,
                ybuf.reshape(-1)[yoff:], ldy, k, s, p, act, scale)
    L.check(rc, "mt_conv2d_fwd")
    x64, w64 = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    conv = F.conv2d(x64, w64, None, (sh, sw), (ph, pw))
    mag = F.conv2d(x64.abs(), w64.abs(), None, (sh, sw), (ph, pw))
    conv, mag = (t.permute(0, 2, 3, 1).reshape(M, K) for t in (conv, mag))
    if b is not None:
        conv, mag = conv + b.double(), mag + b.double().abs()
    if r is not None:
        conv, mag = r[:, :K].double() + scale * conv, r[:, :K].double().abs() + abs(scale) * mag
    y64 = conv.clamp_min(0) if act else conv
    bound = 1.01 * (kh * kw * Cc + 4) * U * mag
    out = ybuf.cpu()
    return out[:, yoff:yoff + K].double(), y64, bound, out


def check(y, y64, bound):
    excess = ((y - y64).abs() - bound).max().item()
    print(f"max err {(y - y64).abs().max().item():.3e}, smallest bound {bound.min().item():.3e}, "
          f"worst err/bound {((y - y64).abs() / bound).max().item():.3f}")
    assert excess <= 0.0, excess


def test_1x1_partial_tile_into_a_channel_slice():
    y, y64, bound, out = run_case(1, 5, 5, 256, 32, yoff=32, ldy=96)
    check(y, y64, bound)
    assert (out[:, :32] == SENTINEL).all() and (out[:, 64:] == SENTINEL).all()


def test_stem_reduction_of_36():
    check(*run_case(2, 9, 9, 4, 32, k=3, s=2)[:3])


def test_3x3_padded_two_faces():
    check(*run_case(2, 3, 3, 32, 32, k=3, p=1)[:3])


@pytest.mark.parametrize("side", [6, 3])
@pytest.mark.parametrize("k,p", [((1, 7), (0, 3)), ((7, 1), (3, 0))])
def test_1x7_and_7x1(side, k, p):
    check(*run_case(2, side, side, 128, 128, k=k, p=p)[:3])


@pytest.mark.parametrize("k,p", [((1, 3), (0, 1)), ((3, 1), (1, 0))])
def test_1x3_and_3x1_on_one_pixel(k, p):
    check(*run_case(3, 1, 1, 192, 192, k=k, p=p)[:3])


def test_k_not_a_multiple_of_the_tile():
    check(*run_case(1, 7, 7, 64, 80)[:3])


def test_reads_a_channel_slice():
    check(*run_case(1, 4, 5, 32, 32, k=3, p=1, xoff=32, ldx=96)[:3])


def test_block_tail_bias_residual_relu():
    y, y64, bound, _ = run_case(1, 6, 7, 96, 256, bias=True, res=True, scale=0.17, act=1)
    check(y, y64, bound)
    assert (y == 0).any() and (y > 0).any()


def test_block8_tail_without_relu_keeps_negative_outputs():
    y, y64, bound, _ = run_case(1, 2, 2, 384, 1792, bias=True, res=True, scale=1.0, act=0)
    check(y, y64, bound)
    assert (y < 0).any()


def test_3x3_stride2_reduction_of_2304():
    check(*run_case(1, 13, 13, 256, 384, k=3, s=2)[:3])


def test_1792_wide_reduction_on_four_rows():
    check(*run_case(1, 2, 2, 1792, 192)[:3])


def test_rows_do_not_depend_on_the_batch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 6, 6, 128, generator=g).cuda()
    w = (torch.randn(128, 3, 3, 128, generator=g) * 0.05).cuda()
    b = torch.randn(128, generator=g).cuda()
    y5 = torch.empty(5 * 36, 128, device="cuda")
    L.check(conv2d(x, 5, 6, 6, 128, 128, w, b, None, 0, y5, 128, 3, 1, 1, 1, 1.0), "mt_conv2d_fwd")
    for n in range(5):
        y1 = torch.empty(36, 128, device="cuda")
        L.check(conv2d(x[n].contiguous(), 1, 6, 6, 128, 128, w, b, None, 0, y1, 128, 3, 1, 1, 1, 1.0), "mt_conv2d_fwd")
        assert torch.equal(y1, y5[n * 36:(n + 1) * 36])


def test_refusals_write_nothing():
    x = torch.randn(1, 5, 5, 8).cuda()
    w = torch.randn(8, 3, 3, 8).cuda()
    y = torch.full((9, 8), SENTINEL).cuda()
    assert conv2d(x, 1, 5, 5, 8, 8, w, None, None, 0, y, 8, 3, 1, 0, 0, 1.0, grid=(4, 3)) == -1          # MT_ERR_ARG
    assert conv2d(x.reshape(-1)[1:], 1, 5, 4, 8, 8, w, None, None, 0, y, 8, 3, 1, 0, 0, 1.0) == -3        # misaligned x
    assert conv2d(x, 1, 5, 5, 8, 8, w.reshape(-1)[2:], None, None, 0, y, 8, 3, 1, 0, 0, 1.0) == -3        # misaligned w
    w6 = torch.randn(6, 3, 3, 8).cuda()
    assert conv2d(x, 1, 5, 5, 8, 8, w6, None, None, 0, y, 8, 3, 1, 0, 0, 1.0) == -3                       # K % 4
    assert conv2d(x, 1, 5, 5, 8, 10, w, None, None, 0, y, 8, 3, 1, 0, 0, 1.0) == -3                       # pitch % 4
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()


# ---- mt_face_ingest ---------------------------------------------------------------------------------------------------------------
def ingest(src, strides, T, H, W, standardize):
    out = torch.full((T, H, W, 4), SENTINEL, device="cuda")
    L.check(L.get().mt_face_ingest(L.ptr(src), int(src.dtype == torch.uint8), *strides, T, H, W, int(standardize), L.ptr(out), L.stream_ptr()),
            "mt_face_ingest")
    return out.cpu()


def test_ingest_uint8_is_the_exact_standardisation():
    g = torch.Generator().manual_seed(1)
    u = torch.randint(0, 256, (3, 5, 7, 3), generator=g, dtype=torch.uint8)
    u[0, 0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    want = (u.float() - 127.5) / 128.0
    out = ingest(u.cuda(), u.stride(), 3, 5, 7, True)                             # channels-last
    assert torch.equal(out[..., :3], want) and (out[..., 3] == 0).all()
    planar = u.permute(0, 3, 1, 2).contiguous()                                    # [T, 3, H, W]
    s = planar.stride()
    out = ingest(planar.cuda(), (s[0], s[2], s[3], s[1]), 3, 5, 7, True)
    assert torch.equal(out[..., :3], want) and (out[..., 3] == 0).all()


def test_ingest_fp32_passthrough_and_raw_fp32():
    g = torch.Generator().manual_seed(2)
    f = torch.randn(2, 4, 6, 3, generator=g)
    out = ingest(f.cuda(), f.stride(), 2, 4, 6, False)
    assert torch.equal(out[..., :3], f) and (out[..., 3] == 0).all()
    planar = f.permute(0, 3, 1, 2).contiguous()
    s = planar.stride()
    out = ingest(planar.cuda(), (s[0], s[2], s[3], s[1]), 2, 4, 6, False)
    assert torch.equal(out[..., :3], f) and (out[..., 3] == 0).all()
    raw = torch.randint(0, 256, (2, 4, 6, 3), generator=g).float()
    out = ingest(raw.cuda(), raw.stride(), 2, 4, 6, True)
    assert torch.equal(out[..., :3], (raw - 127.5) / 128.0)


# ---- mt_maxpool2d_fwd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [7, 8])
def test_maxpool_into_a_slice(side):
    g = torch.Generator().manual_seed(side)
    N, Cc, ldx, ldy, off = 2, 12, 16, 24, 8
    x = torch.randn(N, side, side, Cc, generator=g) - 1.0                          # mostly negative
    xb = torch.full((N * side * side, ldx), 99.0)
    xb[:, :Cc] = x.reshape(-1, Cc)
    so = (side - 3) // 2 + 1
    yb = torch.full((N * so * so, ldy), SENTINEL).cuda()
    L.check(L.get().mt_maxpool2d_fwd(L.ptr(xb.cuda()), ldx, L.ptr(yb.reshape(-1)[off:]), ldy, N, side, side, Cc, 3, 2, 0, L.stream_ptr()),
            "mt_maxpool2d_fwd")
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).reshape(-1, Cc)
    out = yb.cpu()
    assert torch.equal(out[:, off:off + Cc], want)
    assert (out[:, :off] == SENTINEL).all() and (out[:, off + Cc:] == SENTINEL).all()


def test_maxpool_refuses_other_geometries():
    x = torch.zeros(1, 7, 7, 4).cuda()
    y = torch.zeros(9, 4).cuda()
    for k, s, p in ((2, 2, 0), (3, 1, 0), (3, 2, 1)):
        assert L.get().mt_maxpool2d_fwd(L.ptr(x), 4, L.ptr(y), 4, 1, 7, 7, 4, k, s, p, L.stream_ptr()) == -3


# ---- mt_avgpool_rows / mt_l2_normalize_rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 4, 9])
def test_avgpool_rows(rows):
    g = torch.Generator().manual_seed(rows)
    N, Cc, ldx = 3, 1792, 1796
    x = torch.randn(N * rows, ldx, generator=g)
    y = torch.empty(N, Cc, device="cuda")
    L.check(L.get().mt_avgpool_rows(L.ptr(x.cuda()), ldx, L.ptr(y), Cc, N, rows, Cc, L.stream_ptr()), "mt_avgpool_rows")
    x64 = x[:, :Cc].double().reshape(N, rows, Cc)
    want, mag = x64.mean(1), x64.abs().mean(1)
    err = (y.cpu().double() - want).abs()
    print(f"avgpool rows {rows}: worst err / bound {(err / ((rows + 2) * U * mag)).max().item():.3f}")
    assert (err <= (rows + 2) * U * mag).all()


def test_l2_normalize_rows():
    g = torch.Generator().manual_seed(3)
    D = 512
    x = torch.randn(6, D, generator=g)
    x[2] = 0.0
    x[4] *= 1e-3
    y = torch.full((6, D), SENTINEL, device="cuda")
    L.check(L.get().mt_l2_normalize_rows(L.ptr(x.cuda()), D, L.ptr(y), D, 6, D, 1e-12, L.stream_ptr()), "mt_l2_normalize_rows")
    x64 = x.double()
    want = x64 / x64.norm(dim=1, keepdim=True).clamp_min(1e-12)
    out = y.cpu()
    assert (out[2] == 0).all()
    err = (out.double() - want).abs()
    print(f"l2 normalize: worst err / bound {(err[want != 0] / ((D + 2) * U * want.abs()[want != 0])).max().item():.3f}")
    assert (err <= (D + 2) * U * want.abs()).all()
