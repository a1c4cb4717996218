"""Per-kernel parity of the frame extractors' hand-written non-GEMM kernels (csrc/effnet_fwd.hip, csrc/effnet_bwd.hip and the weight
packing of csrc/xception.hip: the depthwise convolution with its two gradients, the BatchNorm bookkeeping, the
activation adjoint, squeeze-excite, the stem weight gradient) against tests/effnet_ops_ref.py in fp64 on the CPU (tied to torch autograd
by tests/test_effnet_ops_ref_host.py).  The conventions are those of tests/test_gpu_tsf_ops.py: every test calls the C ABI directly;
stored outputs start as NaN, accumulated ones (dw, dgamma, dbeta, dw1, dw2, db1, db2) at a canary that the reference adds; outputs sit
between guard bands; figures are printed before anything is asserted; MT_TEST_YARDSTICK=1 prints the error of the same reference
evaluated in fp32 torch on the CPU beside the kernels'.  Comparisons are per SECTION -- border ring and interior, first and last
channel chunk, the worst single image; the two sums separately -- so that a wrong ring, chunk, partial tile or second tile cannot hide
under the maximum of a whole tensor.  The exact checks (canaries, guard bands, refusals, bit-identity of deterministic launches and of
the integer-limb sums, the unpack round trip) have no tolerance; every other gate is twice the worst case measured on an MI355X,
rounded up to one significant digit, with the measured value, its case and the fp32 yardstick of that case beside it.

How each dispatch form was confirmed from the code (csrc/effnet_fwd.hip, csrc/effnet_bwd.hip, csrc/common.hpp):
  * tile size: launch_dw_tiled_any takes 14 x 14 tiles when Ho >= 14, else 7 x 7 (Wo plays no part); launch_dw_bwd_tiled_any decides the
    data gradient (and the fused form) by H >= 14 and the weight gradient by Ho >= 14 -- H 14 at stride 2 gives one of each;
  * chunk width: C % 16 == 0 -> 16-channel chunks, else 8 (C 24 and 40);
  * several tiles per block: xcd_chunk_grid launches 8 * chunks * min(target / (8 * chunks), ceil(tiles / 8)) blocks; at C 1152 (72
    chunks) the forward and the plain data gradient (target 8192) get 14 tile slots per XCD = 112 for the 120 tiles of N 120 at 7 x 7,
    the weight gradient and the fused form (target 4096) 56: blocks walk 2 or 3 tiles with the next one's loads in flight;
  * squeeze-excite: pick_cqb takes the largest divisor of C / 4 up to 64 (C 4, 40, 96, 144, 1152 -> 1, 10, 24, 36, 48; blocks of 256,
    250, 240, 252, 240 threads); se_pool_parts doubles the slices while N * (CQ / CQB) * parts < 2048 and HW / (2 parts) >= 16 PB: two
    slices of 201 and 200 pixels at N 2, HW 401, C 96; mt_se_bwd's reduction slices alike and meets in atomics, or runs unsliced in
    deterministic mode; its weight-gradient kernel takes 16 images per block at these sizes (N 19: 16 + 3, N 35: 16 + 16 + 3) or, in
    deterministic mode, all of them in one block, 16 per LDS chunk;
  * stem weight gradient: the MFMA form for Wo <= 128 outside deterministic mode, else the outer-product kernel (W 258: Wo 129);
  * accumulators: slots > 0 = fp64 atomics into [slots][2][C]; slots < 0 = two integer limbs per accumulator, [2][|slots|][2][C]."""
import os
from contextlib import contextmanager

import pytest
import torch

from mintime_amd import lib as L

from . import effnet_ops_ref as R
from .util import GRAD_TOL_UNIT, rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

CANARY = 7.0
EPS = 1e-3
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3          # csrc/common.hpp
YARD = bool(os.environ.get("MT_TEST_YARDSTICK"))
F64 = torch.float64

# gate = 2 x the worst case measured on an MI355X over every comparison that uses it, one significant digit up.  Beside it: that worst
# case (figure and case), and the yardstick -- the largest error, over the same case's sections, of the same reference evaluated in fp32
# torch on the CPU against fp64.  The largest kernel / yardstick ratio is 4.7 (the forward's channel sums: fp32 block partials of up to
# 196 x tiles values against torch's pairwise sum); nothing comes near the project's ceilings below.
TOL = {
    "dw_fwd.zout": 6e-7,              # 2.7e-7 (worst image, k 5 s 1 swish, N 120 7x7 C 1152); yardstick 2.7e-7
    "dw_fwd.sums": 8e-7,              # 3.7e-7 (sum z, slots 8, k 3 s 2 swish, N 1 30x16 C 24); yardstick 7.8e-8
    "dw_bwd.du_in": 8e-7,             # 3.8e-7 (worst image, parts 2 slots 8, k 5 s 1 swish, N 120 7x7 C 1152); yardstick 3.5e-7
    "dw_bwd.sums": 9e-7,              # 4.4e-7 (sum du_in xhat first chunk, parts 2 + residuals, k 3 s 2 swish, N 2 10x10 C 40); yardstick 1.6e-7
    "dw_bwd.dw": 6e-7,                # 2.9e-7 (last chunk, parts 1, k 5 s 1 swish, N 120 7x7 C 1152); yardstick 1.2e-7
    "se_fwd": 6e-7,                   # 2.6e-7 (hidden, image 1, N 3 HW 49 C 4 CS 5); yardstick 7.6e-8
    "se_bwd.data": 2e-6,              # 5.2e-7 (dpooled, image 0, parts 3, N 3 HW 49 C 4 CS 5); yardstick 3.0e-7
    "se_bwd.wgrad": 5e-7,             # 2.4e-7 (dw1, deterministic, N 35 HW 49 C 144 CS 28); yardstick 2.0e-7
    "bn_finalize": 3e-7,              # 1.2e-7 (shift, C 1152 slots 32 training count 300); yardstick 1.3e-6 (fp32 Q / count - m^2)
    "bn_bwd_finalize.kabc": 3e-7,     # 1.4e-7 (kb, C 40 slots 32 training); yardstick 1.4e-7
    "bn_bwd_finalize.grads": 2e-7,    # 7.4e-8 (dbeta on its canary, C 24 slots -32 training); yardstick 3.1e-8
    "bn_act_fwd": 3e-7,               # 1.1e-7 (last 4 channels, swish, rows 3300 C 1280); yardstick 1.2e-7
    "bn_act_bwd.du": 4e-7,            # 2.0e-7 (middle images, swish + gate + rowscale, rows 3500 hw 49 C 1152); yardstick 1.7e-7
    "bn_act_bwd.sums": 3e-7,          # 1.3e-7 (sum du xhat, swish, rows 258 hw 49 C 24 slots 8); yardstick 9.4e-8
    "stem_wgrad": 5e-7,               # 2.3e-7 (dw[:, :, 2, :], 8x12 uint8 crops, deterministic); yardstick 2.1e-7
}
# no gate looser than what the project already accepts for the same kind of quantity
_CEILING = {"zout": 2e-5, "du_in": 2e-5, "du": 2e-5, "data": 2e-5, "sums": 1e-4, "dw": GRAD_TOL_UNIT, "wgrad": GRAD_TOL_UNIT,
            "grads": GRAD_TOL_UNIT, "stem_wgrad": GRAD_TOL_UNIT, "se_fwd": 1e-5, "bn_finalize": 1e-5, "kabc": 1e-5, "bn_act_fwd": 1e-5}
assert all(v <= _CEILING[k.split(".")[-1]] for k, v in TOL.items())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return t.contiguous().to(dev)


@contextmanager
def _det(on):
    prev = L.set_deterministic(on)
    try:
        yield
    finally:
        L.set_deterministic(prev)


def _guarded(numel, fill=float("nan"), dtype=torch.float32):
    """A device buffer of `numel` elements holding `fill`, between two 64-element guard bands of -0.0 (any store shows in them, and so
    does a read-modify-write that adds +0.0)."""
    buf = torch.full((numel + 128,), -0.0, dtype=dtype, device=dev)
    body = buf[64:64 + numel]
    body.fill_(fill)
    return buf, body


def _bands_intact(buf):
    bits = buf.view(torch.int64 if buf.dtype == F64 else torch.int32)
    guard = -2 ** 63 if buf.dtype == F64 else -2 ** 31
    return bool((bits[:64] == guard).all() and (bits[-64:] == guard).all())


class _Figures:
    """Collects the figures of one test, prints each before anything is asserted, then fails on all that missed.  yard = True: the
    same comparisons for the fp32 CPU evaluation of the reference, printed only."""

    def __init__(self, what, yard=False):
        self.what, self.bad, self.is_yard = what, [], yard

    def close(self, kind, name, got, ref):
        return self.value(kind, name, rel_err(got, ref))

    def value(self, kind, name, e):
        if self.is_yard:
            print(f"YARD {kind} | {self.what} | {name} | {e:.3e}")
            return e
        print(f"FIG {kind} | {self.what} | {name} | {e:.3e} | tol {TOL[kind]:.0e}")
        if not e <= TOL[kind]:
            self.bad.append(f"{name}: {e:.3e} > {TOL[kind]:.0e}")
        return e

    def true(self, name, cond):
        if not bool(cond):
            print(f"FIG exact | {self.what} | {name} | FALSE")
            self.bad.append(name)

    def done(self):
        assert not self.bad, f"{self.what}: " + "; ".join(self.bad)


def _spatial(fig, kind, name, got, ref, N, H, W, ring, cc):
    """[N*H*W, C] rows compared per section: border ring (width `ring`) / interior, first / last `cc` channels, the worst image."""
    C = ref.shape[-1]
    g, r = got.detach().cpu().double().reshape(N, H, W, C), ref.double().reshape(N, H, W, C)
    edge = torch.ones(H, W, dtype=torch.bool)
    edge[ring:H - ring, ring:W - ring] = False
    fig.close(kind, f"{name} border ring", g[:, edge], r[:, edge])
    if not bool(edge.all()):
        fig.close(kind, f"{name} interior", g[:, ~edge], r[:, ~edge])
    fig.close(kind, f"{name} first chunk", g[..., :cc], r[..., :cc])
    fig.close(kind, f"{name} last chunk", g[..., C - cc:], r[..., C - cc:])
    worst = ((g - r).abs().amax(dim=(1, 2, 3)) / r.abs().amax(dim=(1, 2, 3)).clamp_min(1e-30)).max()
    fig.value(kind, f"{name} worst image", float(worst))


def _sums(fig, kind, name, got, ref, cc):
    """Per-channel sums [C]: whole, first and last channel chunk."""
    C = ref.shape[-1]
    fig.close(kind, name, got, ref)
    fig.close(kind, f"{name} first chunk", got[..., :cc], ref[..., :cc])
    fig.close(kind, f"{name} last chunk", got[..., C - cc:], ref[..., C - cc:])


def _stats_buffer(slots, C):
    """Zeroed accumulators for `slots` as the ABI defines them: [|slots|][2][C] fp64, twice that (two integer limbs) when negative."""
    return _guarded((2 if slots < 0 else 1) * abs(slots) * 2 * C, 0.0, F64)


def _stats_read(body, slots, C):
    """[2][C] totals over the slots; the limb form decoded as stat_get does: hi + lo * 2^-44 per slot."""
    if slots > 0:
        return body.reshape(slots, 2, C).sum(0).cpu()
    limbs = body.view(torch.int64).reshape(2, -slots, 2, C).cpu()
    return (limbs[0].double() + limbs[1].double() * 2.0 ** -44).sum(0)


def _to(dtype, *ts):
    return [None if t is None else t.to(dtype) for t in ts]


# ---- 1. mt_dwconv_fwd ------------------------------------------------------------------------------------------------------------

KSA = [(k, s, a) for k in (3, 5) for s in (1, 2) for a in (0, 1, 2)]
# (N, H, W, C): what the shape reaches at stride 1 / stride 2
DW_FWD_SHAPES = [(2, 15, 15, 48),      # Ho 15: 14-tiles with partial last tiles / Ho 8: 7-tiles, partial; odd H at stride 2; 16-channel chunks
                 (1, 19, 19, 24),      # Ho 19 / Ho 10 (7-tiles, partial), odd H at stride 2; 8-channel chunks
                 (2, 10, 10, 40),      # Ho 10: 7-tiles, partial / Ho 5; 8-channel chunks
                 (1, 9, 20, 48),       # H != W: Ho 9 takes 7-tiles over Wo 20 / Ho 5, Wo 10, and at stride 2 the odd H pads (k - 1) / 2
                                       # in front but the even W (k - 2) / 2 (the kernel once used H's pad for both axes)
                 (1, 30, 16, 24),      # H != W: Ho 30, Wo 16 / Ho 15 (14-tiles), Wo 8
                 (1, 7, 7, 48),        # one tile: most of the grid's blocks own none and must add nothing to the sums
                 (2, 28, 28, 48)]      # full tiles only / Ho 14: exactly one 14-tile per image


def _cc(C):
    return 16 if C % 16 == 0 else 8


def _off_the_kink(z, scale, shift):
    """z with the elements moved whose u = z scale + shift lies within 1e-3 of 0: relu' jumps there, and fp32 and fp64 may disagree
    about the side -- a difference of the reference's making, not the kernel's."""
    u = z.double() * scale.double() + shift.double()
    return torch.where(u.abs() < 1e-3, z + (0.01 / scale), z)


def _dw_inputs(N, H, W, C, k, s, seed):
    g = _gen(seed)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    zin = _off_the_kink(torch.randn(N * H * W, C, generator=g), scale, shift)
    w = torch.randn(C, 1, k, k, generator=g) * 0.3 + 0.15          # taps with a non-zero mean: the channel sums do not cancel
    return zin, scale, shift, w


def _dw_fwd_launch(zin_d, scale_d, shift_d, w_d, N, H, W, C, k, s, act, slots):
    Ho, Wo = -(-H // s), -(-W // s)
    obuf, zout = _guarded(N * Ho * Wo * C)
    sbuf, st = _stats_buffer(slots, C) if slots else (None, None)
    L.check(L.get().mt_dwconv_fwd(L.ptr(zin_d), L.ptr(scale_d), L.ptr(shift_d), L.ptr(w_d), L.ptr(zout), L.ptr(st), slots, N, H, W, C,
                                  k, s, act, L.stream_ptr()), "mt_dwconv_fwd")
    torch.cuda.synchronize()
    assert _bands_intact(obuf) and (sbuf is None or _bands_intact(sbuf)), "mt_dwconv_fwd wrote outside its outputs"
    return zout, st


def _dw_fwd_compare(fig, zout, sums, ref, N, Ho, Wo, C, k):
    _spatial(fig, "dw_fwd.zout", "mt_dwconv_fwd zout", zout, ref[0], N, Ho, Wo, (k - 1) // 2, _cc(C))
    for tag, st in sums:
        _sums(fig, "dw_fwd.sums", f"mt_dwconv_fwd sum z ({tag})", st[0], ref[1], _cc(C))
        _sums(fig, "dw_fwd.sums", f"mt_dwconv_fwd sum z^2 ({tag})", st[1], ref[2], _cc(C))


def _dw_fwd_check(N, H, W, C, k, s, act, seed=0):
    zin, scale, shift, w = _dw_inputs(N, H, W, C, k, s, 1000 * k + 100 * s + 10 * act + H + seed)
    Ho, Wo = -(-H // s), -(-W // s)
    ref = R.dw_fwd(*_to(F64, zin, scale, shift, w), N, H, W, k, s, act)
    what = f"dw_fwd k{k} s{s} act{act} N{N} {H}x{W} C{C}"
    if YARD:
        r32 = R.dw_fwd(zin, scale, shift, w, N, H, W, k, s, act)
        _dw_fwd_compare(_Figures(what, True), r32[0], [("fp32", torch.stack(r32[1:]))], ref, N, Ho, Wo, C, k)
    dv = [_d(t) for t in (zin, scale, shift, w)]
    fig = _Figures(what)
    zout, _ = _dw_fwd_launch(*dv, N, H, W, C, k, s, act, 0)                 # stats = NULL
    z8, st8 = _dw_fwd_launch(*dv, N, H, W, C, k, s, act, 8)
    zl, stl = _dw_fwd_launch(*dv, N, H, W, C, k, s, act, -8)
    zl2, stl2 = _dw_fwd_launch(*dv, N, H, W, C, k, s, act, -8)
    _dw_fwd_compare(fig, zout, [("slots 8", _stats_read(st8, 8, C)), ("slots -8", _stats_read(stl, -8, C))], ref, N, Ho, Wo, C, k)
    fig.true("zout has no NaN left", not bool(torch.isnan(zout).any()))
    fig.true("zout is the same bits with and without statistics", torch.equal(zout, z8) and torch.equal(zout, zl))
    fig.true("the limb sums of two launches are the same bits", torch.equal(stl.view(torch.int64), stl2.view(torch.int64)))
    fig.done()


@pytest.mark.parametrize("N,H,W,C", DW_FWD_SHAPES)
@pytest.mark.parametrize("k,s,act", KSA)
def test_depthwise_forward_vs_fp64(k, s, act, N, H, W, C):
    """mt_dwconv_fwd: zout per section and its BatchNorm sums (sum, sum of squares separately; no statistics, fp64 slots, integer
    limbs) against R.dw_fwd in fp64."""
    _dw_fwd_check(N, H, W, C, k, s, act)


def test_depthwise_forward_second_tile_of_a_block():
    """N 120 at 7 x 7, C 1152, k 5: 120 tiles for the 112 tile slots of the grid (module docstring), so sixteen blocks of every
    channel chunk convolve a second tile whose loads were issued under the first."""
    _dw_fwd_check(120, 7, 7, 1152, 5, 1, 1)


def test_depthwise_forward_limb_sums_of_negative_and_small_partials():
    """The integer-limb accumulators by value where truncation matters: channels whose outputs average -3 (negative block partials:
    trunc rounds towards zero, the fraction limb is negative), +3, and +-3e-3 (block partials below 1 in magnitude: limb 0 gets 0)."""
    N, H, W, C, k, s = 3, 15, 15, 48, 3, 1
    g = _gen(77)
    zin = torch.randn(N * H * W, C, generator=g) * 0.3
    sign = torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    small = torch.arange(C) % 3 == 2
    small_sign = torch.where(torch.arange(C) % 2 == 0, -1.0, 1.0)
    scale = torch.where(small, torch.full((C,), 1e-3), torch.ones(C))
    shift = torch.where(small, 3e-3 * small_sign, 3.0 * sign)
    w = torch.full((C, 1, k, k), 1.0 / 9) + torch.randn(C, 1, k, k, generator=g) * 0.02
    ref = R.dw_fwd(*_to(F64, zin, scale, shift, w), N, H, W, k, s, 0)
    mean = ref[1] / (N * H * W)
    assert float(mean[0]) < -2 and float(mean[1]) > 2 and float(ref[0][:, small].reshape(N, -1, int(small.sum())).abs().sum(1).max()) < 1.0      # (one block = at most one tile of one image here)
    fig = _Figures("dw_fwd limb sums, means -3 / +3 / +-3e-3")
    groups = (("mean -3", torch.arange(C) % 3 == 0), ("mean +3", torch.arange(C) % 3 == 1), ("sums below 1", small))
    if YARD:
        r32 = R.dw_fwd(zin, scale, shift, w, N, H, W, k, s, 0)
        for tag, m in groups:
            _Figures(fig.what, True).close("dw_fwd.sums", f"sum z, {tag}", r32[1][m], ref[1][m])
            _Figures(fig.what, True).close("dw_fwd.sums", f"sum z^2, {tag}", r32[2][m], ref[2][m])
    dv = [_d(t) for t in (zin, scale, shift, w)]
    _, st = _dw_fwd_launch(*dv, N, H, W, C, k, s, 0, -8)
    _, st2 = _dw_fwd_launch(*dv, N, H, W, C, k, s, 0, -8)
    got = _stats_read(st, -8, C)
    for tag, m in groups:
        fig.close("dw_fwd.sums", f"mt_dwconv_fwd limb sum z, {tag}", got[0][m], ref[1][m])
        fig.close("dw_fwd.sums", f"mt_dwconv_fwd limb sum z^2, {tag}", got[1][m], ref[2][m])
    limbs = st.view(torch.int64).reshape(2, 8, 2, C).cpu()
    fig.true("limb 0 of the small channels holds 0", (limbs[0][:, :, small] == 0).all())
    fig.true("the negative channels have negative limbs", (limbs[0][:, 0, 0].sum(0) < 0) and (limbs[1][:, 0, 0] <= 0).all())
    fig.true("the limb sums of two launches are the same bits", torch.equal(st.view(torch.int64), st2.view(torch.int64)))
    fig.done()


# ---- 2. mt_dwconv_bwd / mt_dwconv_bwd_res2 -----------------------------------------------------------------------------------------

DW_BWD_SHAPES = {1: DW_FWD_SHAPES[:6],
                 2: [(2, 14, 14, 48),      # the data gradient tiles by H (14-tiles), the weight gradient by Ho = 7 (7-tiles)
                     (1, 20, 12, 24),      # H != W; 8-channel chunks; Ho 10 x Wo 6
                     (2, 10, 10, 40),      # 7-tiles both ways, partial
                     (1, 30, 16, 24),      # Ho 15: partial 14-tiles in the weight gradient
                     (1, 28, 28, 48)]}


def _dw_bwd_inputs(N, H, W, C, k, s, seed, half_res=False):
    zin, scale, shift, w = _dw_inputs(N, H, W, C, k, s, seed)
    g = _gen(seed + 1)
    Ho, Wo = -(-H // s), -(-W // s)
    du = torch.randn(N * Ho * Wo, C, generator=g) + 0.5              # a non-zero mean: the sums of du_in do not cancel
    z = torch.randn(N * Ho * Wo, C, generator=g)
    kabc = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1])
    mi = torch.stack([torch.randn(C, generator=g) * 0.5 + 1.0, torch.rand(C, generator=g) + 0.5])   # off-centre: xhat has a mean
    rrows = N * ((H + 1) // 2) * ((W + 1) // 2) if half_res else N * H * W
    res_pre, res_post = torch.randn(rrows, C, generator=g), torch.randn(rrows, C, generator=g)
    return {"du": du, "z": z, "kabc": kabc, "w": w, "zin": zin, "scale": scale, "shift": shift, "mi": mi, "res_pre": res_pre,
            "res_post": res_post}


def _dw_bwd_ref(c, dtype, N, H, W, k, s, act, res, stats=True, half_res=False):
    t = {n: v.to(dtype) for n, v in c.items()}
    rp, rq = (t["res_pre"], t["res_post"]) if res else (None, None)
    if res and half_res:
        rp, rq = R.half_to_full(rp, N, H, W), R.half_to_full(rq, N, H, W)
    return R.dw_bwd(t["du"], t["z"], t["kabc"], t["w"], t["zin"], t["scale"], t["shift"], t["mi"] if stats else None, N, H, W, k, s,
                    act, rp, rq)


def _dw_bwd_launch(cd, N, H, W, C, k, s, act, parts, slots, res, fn="mt_dwconv_bwd"):
    """One launch; du_in [N*H*W, C] or None, the totals of the sums or None, dw minus nothing (it starts at the canary) or None."""
    ibuf, du_in = _guarded(N * H * W * C) if parts & 2 else (None, None)
    sbuf, st = _stats_buffer(slots, C) if (parts & 2) and slots else (None, None)
    wbuf, dw = _guarded(C * k * k, CANARY) if parts & 1 else (None, None)
    rc = getattr(L.get(), fn)(L.ptr(cd["du"]), L.ptr(cd["z"]), L.ptr(cd["kabc"]), L.ptr(cd["w"]), L.ptr(cd["zin"]), L.ptr(cd["scale"]),
                              L.ptr(cd["shift"]), L.ptr(cd["mi"]) if st is not None else None, L.ptr(du_in), L.ptr(st), slots,
                              L.ptr(dw), N, H, W, C, k, s, parts, act, L.ptr(cd["res_pre"]) if res else None,
                              L.ptr(cd["res_post"]) if res else None, L.stream_ptr())
    L.check(rc, fn)
    torch.cuda.synchronize()
    assert all(b is None or _bands_intact(b) for b in (ibuf, sbuf, wbuf)), f"{fn} wrote outside its outputs"
    return du_in, (None if st is None else _stats_read(st, slots, C)), (None if dw is None else dw.reshape(C, 1, k, k)), st


def _dw_bwd_compare(fig, tag, du_in, sums, dw, ref, N, H, W, C, k, kinds=("dw_bwd.du_in", "dw_bwd.sums", "dw_bwd.dw"), canary=CANARY):
    if du_in is not None:
        _spatial(fig, kinds[0], f"{tag} du_in", du_in, ref[0], N, H, W, (k - 1) // 2, _cc(C))
    if sums is not None:
        _sums(fig, kinds[1], f"{tag} sum du_in", sums[0], ref[1], _cc(C))
        _sums(fig, kinds[1], f"{tag} sum du_in xhat", sums[1], ref[2], _cc(C))
    if dw is not None:
        fig.close(kinds[2], f"{tag} dw (on the canary)", dw, ref[3] + canary)
        fig.close(kinds[2], f"{tag} dw first chunk", dw[:_cc(C)], ref[3][:_cc(C)] + canary)
        fig.close(kinds[2], f"{tag} dw last chunk", dw[-_cc(C):], ref[3][-_cc(C):] + canary)


def _dw_bwd_check(N, H, W, C, k, s, act, seed=0, residuals=True):
    c = _dw_bwd_inputs(N, H, W, C, k, s, 2000 * k + 200 * s + 20 * act + H + seed)
    ref_res = _dw_bwd_ref(c, F64, N, H, W, k, s, act, True) if residuals else None
    ref = _dw_bwd_ref(c, F64, N, H, W, k, s, act, False)
    what = f"dw_bwd k{k} s{s} act{act} N{N} {H}x{W} C{C}"
    if YARD:
        if residuals:
            y = _dw_bwd_ref(c, torch.float32, N, H, W, k, s, act, True)
            _dw_bwd_compare(_Figures(what, True), "fp32 with residuals", y[0], torch.stack(y[1:3]), y[3], ref_res, N, H, W, C, k, canary=0.0)
        y = _dw_bwd_ref(c, torch.float32, N, H, W, k, s, act, False)
        _dw_bwd_compare(_Figures(what, True), "fp32", y[0], torch.stack(y[1:3]), y[3], ref, N, H, W, C, k, canary=0.0)
    cd = {n: _d(v) for n, v in c.items()}
    fig = _Figures(what)
    du_in, sums, _, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, act, 2, 8, residuals)
    _dw_bwd_compare(fig, f"mt_dwconv_bwd parts 2{' + residuals' * residuals}, slots 8:", du_in, sums, None, ref_res if residuals else ref,
                    N, H, W, C, k)
    fig.true("parts 2: du_in has no NaN left", not bool(torch.isnan(du_in).any()))
    _, _, dw, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, act, 1, 0, False)
    _dw_bwd_compare(fig, "mt_dwconv_bwd parts 1:", None, None, dw, ref, N, H, W, C, k)
    du_in3, sums3, dw3, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, act, 3, -8, False)
    _dw_bwd_compare(fig, "mt_dwconv_bwd parts 3, slots -8:", du_in3, sums3, dw3, ref, N, H, W, C, k)
    if not residuals:
        return fig.done()
    du_in0, _, _, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, act, 2, 0, False)        # stats_in = mean_invstd_in = NULL
    _dw_bwd_compare(fig, "mt_dwconv_bwd parts 2, no sums:", du_in0, None, None, ref, N, H, W, C, k)
    du_in3r, sums3r, dw3r, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, act, 3, 8, True)
    _dw_bwd_compare(fig, "mt_dwconv_bwd parts 3 + residuals, slots 8:", du_in3r, sums3r, dw3r, ref_res, N, H, W, C, k)
    fig.done()


@pytest.mark.parametrize("k,s,act,N,H,W,C", [(k, s, a) + shp for (k, s, a) in KSA for shp in DW_BWD_SHAPES[s]])
def test_depthwise_backward_vs_fp64(k, s, act, N, H, W, C):
    """mt_dwconv_bwd parts 1, 2 and 3: du_in per section with and without res_pre / res_post, the BatchNorm-backward sums (sum du_in
    and sum du_in xhat separately, fp64 slots and integer limbs, and none), dw on its canary -- all against R.dw_bwd in fp64."""
    _dw_bwd_check(N, H, W, C, k, s, act)


def test_depthwise_backward_several_tiles_per_block():
    """N 120 at 7 x 7, C 1152, k 5: 120 tiles for 112 tile slots in the plain data gradient and for 56 in the weight gradient and
    the fused form (module docstring): second and third tiles of a block, prefetched under the one before."""
    _dw_bwd_check(120, 7, 7, 1152, 5, 1, 1, residuals=False)


@pytest.mark.parametrize("k,s,N,H,W,C", [(3, 1, 2, 15, 15, 48), (5, 2, 2, 14, 14, 48), (3, 2, 1, 30, 16, 24)])
def test_depthwise_weight_gradient_deterministic(k, s, N, H, W, C):
    """Deterministic mode: the parts = 1 weight gradient (fixed-order reduction of the blocks' partials) against fp64, and the same
    bits from two launches."""
    c = _dw_bwd_inputs(N, H, W, C, k, s, 31 * k + s)
    ref = _dw_bwd_ref(c, F64, N, H, W, k, s, 1, False)
    cd = {n: _d(v) for n, v in c.items()}
    fig = _Figures(f"dw_bwd deterministic k{k} s{s} N{N} {H}x{W} C{C}")
    with _det(True):
        _, _, dw, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, 1, 1, 0, False)
        _, _, dw2, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, 1, 1, 0, False)
    _dw_bwd_compare(fig, "mt_dwconv_bwd parts 1, deterministic:", None, None, dw, ref, N, H, W, C, k)
    fig.true("two deterministic launches give the same bits", torch.equal(dw, dw2))
    fig.done()


@pytest.mark.parametrize("k,act,H,W,C", [(3, 2, 19, 19, 24), (3, 0, 10, 10, 48), (5, 2, 19, 10, 40), (3, 1, 10, 19, 48)])
def test_depthwise_backward_half_resolution_residuals_vs_fp64(k, act, H, W, C):
    """mt_dwconv_bwd_res2: res_pre / res_post given at the even (ih, iw) only, [N, ceil(H/2), ceil(W/2), C], odd and even H / W."""
    N, s = 2, 1
    c = _dw_bwd_inputs(N, H, W, C, k, s, 5000 + 10 * k + H, half_res=True)
    ref = _dw_bwd_ref(c, F64, N, H, W, k, s, act, True, half_res=True)
    what = f"dw_bwd_res2 k{k} act{act} N{N} {H}x{W} C{C}"
    if YARD:
        y = _dw_bwd_ref(c, torch.float32, N, H, W, k, s, act, True, half_res=True)
        _dw_bwd_compare(_Figures(what, True), "fp32", y[0], torch.stack(y[1:3]), y[3], ref, N, H, W, C, k, canary=0.0)
    cd = {n: _d(v) for n, v in c.items()}
    fig = _Figures(what)
    for parts in (2, 3):
        du_in, sums, dw, _ = _dw_bwd_launch(cd, N, H, W, C, k, s, act, parts, 8, True, fn="mt_dwconv_bwd_res2")
        _dw_bwd_compare(fig, f"mt_dwconv_bwd_res2 parts {parts}:", du_in, sums, dw, ref, N, H, W, C, k)
    # the full-resolution entry point afterwards: the half-resolution switch does not outlive its call
    full = dict(cd, res_pre=_d(R.half_to_full(c["res_pre"], N, H, W)), res_post=_d(R.half_to_full(c["res_post"], N, H, W)))
    du_in, sums, _, _ = _dw_bwd_launch(full, N, H, W, C, k, s, act, 2, 8, True)
    _dw_bwd_compare(fig, "mt_dwconv_bwd after it, zero-filled residuals:", du_in, sums, None, ref, N, H, W, C, k)
    fig.done()


def _scratch(numel=1 << 16):
    return torch.zeros(numel, device=dev)


def test_depthwise_refusals():
    """Every argument below is rejected by a host-side check before anything is launched; the buffers are large enough all the same."""
    lib, b, st = L.get(), _scratch(), torch.zeros(1 << 12, dtype=F64, device=dev)
    p, sp, s = L.ptr(b), L.ptr(st), L.stream_ptr()

    def bwd(fn, H, W, C, k, stride):
        return getattr(lib, fn)(p, p, p, p, p, p, p, p, p, sp, 1, p, 1, H, W, C, k, stride, 3, 1, None, None, s)

    assert bwd("mt_dwconv_bwd", 9, 8, 16, 3, 2) == MT_ERR_UNSUPPORTED          # odd H at stride 2
    assert bwd("mt_dwconv_bwd", 8, 9, 16, 5, 2) == MT_ERR_UNSUPPORTED          # odd W at stride 2
    assert bwd("mt_dwconv_bwd", 8, 8, 16, 7, 1) == MT_ERR_UNSUPPORTED          # k 7
    assert bwd("mt_dwconv_bwd", 8, 8, 16, 3, 3) == MT_ERR_UNSUPPORTED          # stride 3
    assert bwd("mt_dwconv_bwd", 8, 8, 12, 3, 1) == MT_ERR_UNSUPPORTED          # C % 8 != 0
    assert bwd("mt_dwconv_bwd_res2", 8, 8, 16, 3, 2) == MT_ERR_UNSUPPORTED     # half-resolution residuals at stride 2
    assert lib.mt_dwconv_bwd(p, p, p, p, p, p, p, None, p, sp, 1, p, 1, 8, 8, 16, 3, 1, 2, 1, None, None, s) == MT_ERR_ARG   # sums without mean_invstd
    assert lib.mt_dwconv_fwd(p, p, p, p, p, None, 0, 1, 8, 8, 12, 3, 1, 1, s) == MT_ERR_ARG            # C % 8 != 0
    assert lib.mt_dwconv_fwd(p, p, p, p, p, None, 0, 1, 8, 8, 16, 3, 1, 3, s) == MT_ERR_ARG            # act 3
    assert lib.mt_dwconv_fwd(p, p, p, p, p, None, 0, 1, 8, 8, 16, 4, 1, 1, s) == MT_ERR_UNSUPPORTED    # k 4
    assert b.abs().sum().item() == 0.0 and st.abs().sum().item() == 0.0


# ---- 3. squeeze-excite forward -------------------------------------------------------------------------------------------------------

SE_C = [4, 40, 96, 144, 1152]                 # block shapes 1 x 256, 10 x 25, 24 x 10, 36 x 7, 48 x 5; 144 = a partial second 128-channel slab
SE_CS = [4, 5, 6, 10, 20, 28, 48]             # odd CS in the two-halves split, CS % 4 != 0 in the four-row walk, CS > 16: two hidden blocks
SE_SHAPES = [(3, 49, C, CS) for C in SE_C for CS in SE_CS] + [(2, 401, 96, 4), (2, 401, 96, 28)]      # (N, HW, C, CS)


def _se_inputs(N, HW, C, CS, seed):
    g = _gen(seed)
    z = torch.randn(N * HW, C, generator=g)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.5
    w1, b1 = torch.randn(CS, C, generator=g) * C ** -0.5, torch.randn(CS, generator=g) * 0.5
    w2, b2 = torch.randn(C, CS, generator=g) * CS ** -0.5, torch.randn(C, generator=g) * 0.5
    da = torch.randn(N * HW, C, generator=g) + 0.3
    return {"z": z, "scale": scale, "shift": shift, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "da": da}


def _se_fwd_ref(c, dtype, N, HW):
    t = {n: v.to(dtype) for n, v in c.items()}
    return R.se_fwd(t["z"], t["scale"], t["shift"], t["w1"], t["b1"], t["w2"], t["b2"], N, HW)


def _se_fwd_launch(cd, N, HW, C, CS, with_pooled=True):
    lib = L.get()
    parts = lib.mt_se_pool_parts(N, HW, C)
    qbuf, partial = _guarded(N * parts * C)
    L.check(lib.mt_se_pool_fwd(L.ptr(cd["z"]), L.ptr(cd["scale"]), L.ptr(cd["shift"]), L.ptr(partial), N, HW, C, parts, L.stream_ptr()),
            "mt_se_pool_fwd")
    pbuf, pooled = _guarded(N * C) if with_pooled else (None, None)
    gbuf, gate = _guarded(N * C)
    hbuf, hidden = _guarded(N * CS)
    L.check(lib.mt_se_gate_fwd(L.ptr(partial), parts, L.ptr(cd["w1"]), L.ptr(cd["b1"]), L.ptr(cd["w2"]), L.ptr(cd["b2"]), L.ptr(pooled),
                               L.ptr(gate), L.ptr(hidden), N, C, CS, L.stream_ptr()), "mt_se_gate_fwd")
    torch.cuda.synchronize()
    assert all(b is None or _bands_intact(b) for b in (qbuf, pbuf, gbuf, hbuf)), "the squeeze-excite forward wrote outside its outputs"
    return parts, partial.reshape(N, parts, C), pooled, hidden.reshape(N, CS), gate.reshape(N, C)


@pytest.mark.parametrize("N,HW,C,CS", SE_SHAPES)
def test_squeeze_excite_forward_vs_fp64(N, HW, C, CS):
    """mt_se_pool_fwd (the slices summed on the host: its own output) and mt_se_gate_fwd's pooled, hidden and gate against R.se_fwd in
    fp64, per image; pooled = NULL gives the same hidden and gate."""
    c = _se_inputs(N, HW, C, CS, 10 * C + CS + HW)
    ref = _se_fwd_ref(c, F64, N, HW)
    what = f"se_fwd N{N} HW{HW} C{C} CS{CS}"
    if YARD:
        for name, y32, r in zip(("pooled", "hidden", "gate"), _se_fwd_ref(c, torch.float32, N, HW), ref):
            _Figures(what, True).close("se_fwd", name, y32, r)
    cd = {n: _d(v) for n, v in c.items()}
    fig = _Figures(what)
    parts, partial, pooled, hidden, gate = _se_fwd_launch(cd, N, HW, C, CS)
    fig.true("N 2, HW 401, C 96 is sliced", parts > 1 or HW != 401)
    fig.true("HW 49 is not sliced", parts == 1 or HW != 49)
    for n in range(N):
        fig.close("se_fwd", f"mt_se_pool_fwd partial sums, image {n}", partial[n].double().sum(0).cpu(), ref[0][n])
        fig.close("se_fwd", f"mt_se_gate_fwd pooled, image {n}", pooled.reshape(N, C)[n], ref[0][n])
        fig.close("se_fwd", f"mt_se_gate_fwd hidden, image {n}", hidden[n], ref[1][n])
        fig.close("se_fwd", f"mt_se_gate_fwd gate, image {n}", gate[n], ref[2][n])
    fig.close("se_fwd", "mt_se_gate_fwd gate, last slab", gate[:, -(C % 128 or 128):], ref[2][:, -(C % 128 or 128):])
    _, _, _, hidden2, gate2 = _se_fwd_launch(cd, N, HW, C, CS, with_pooled=False)
    fig.true("pooled = NULL: same hidden and gate", torch.equal(hidden, hidden2) and torch.equal(gate, gate2))
    fig.done()


def test_squeeze_excite_forward_refusals():
    """Host-side checks only.  mt_se_gate_fwd reserves no LDS beyond what a launch may take unasked, so it admits the squeeze widths
    that fit (1 .. 48, EfficientNet-B0's widest and mt_se_bwd's limit) and refuses the first one outside before any launch."""
    lib, b = L.get(), _scratch()
    p, s = L.ptr(b), L.stream_ptr()
    assert lib.mt_se_pool_parts(2, 401, 96) == 2 and lib.mt_se_pool_parts(3, 49, 96) == 1
    assert lib.mt_se_pool_fwd(p, p, p, p, 2, 401, 96, 1, s) == MT_ERR_ARG          # parts other than mt_se_pool_parts returns
    assert lib.mt_se_pool_fwd(p, p, p, p, 2, 401, 96, 4, s) == MT_ERR_ARG
    assert lib.mt_se_pool_fwd(p, p, p, p, 3, 49, 96, 2, s) == MT_ERR_ARG
    assert lib.mt_se_pool_fwd(p, p, p, p, 3, 49, 6, 1, s) == MT_ERR_ARG            # C % 4 != 0
    assert lib.mt_se_gate_fwd(p, 1, p, p, p, p, p, p, p, 2, 96, 49, s) == MT_ERR_UNSUPPORTED
    assert lib.mt_se_gate_fwd(p, 1, p, p, p, p, p, p, p, 2, 96, 0, s) == MT_ERR_UNSUPPORTED
    assert lib.mt_se_gate_fwd(p, 1, p, p, p, p, p, p, None, 2, 96, 4, s) == MT_ERR_ARG      # hidden is required
    assert b.abs().sum().item() == 0.0


# ---- 4. mt_se_bwd ------------------------------------------------------------------------------------------------------------------

SE_BWD_SHAPES = SE_SHAPES + [(19, 49, 40, 10), (35, 49, 144, 28), (19, 9, 1152, 48)]       # N 19 / 35: 16-image chunks with a ragged last one
_SE_DATA = ("dgate", "dpre2", "dhid", "dpooled")
_SE_WGRAD = ("dw1", "db1", "dw2", "db2")


def _se_bwd_ref(c, fwd, dtype, N, HW, dgate=None):
    """fwd = (pooled, hidden, gate) in fp32: the kernel's inputs, the same values for every evaluation."""
    t = {n: v.to(dtype) for n, v in c.items()}
    pooled, hidden, gate = (v.to(dtype) for v in fwd)
    return R.se_bwd(t["da"], t["z"], t["scale"], t["shift"], gate, hidden, pooled, t["w1"], t["w2"], N, HW,
                    None if dgate is None else dgate.to(dtype))


def _se_bwd_launch(cd, fwd, N, HW, C, CS, mask, dgate_in=None):
    lib = L.get()
    sizes = {"dgate": N * C, "dpre2": N * C, "dhid": N * CS, "dpooled": N * C, "dw1": CS * C, "db1": CS, "dw2": C * CS, "db2": C}
    bufs = {n: _guarded(sz, CANARY if n in _SE_WGRAD else float("nan")) for n, sz in sizes.items()}
    if dgate_in is not None:
        bufs["dgate"][1].copy_(dgate_in.reshape(-1))
    xbuf, scratch = _guarded(lib.mt_se_scratch_floats(N, C, CS))
    o = {n: b[1] for n, b in bufs.items()}
    first = mask & 1
    L.check(lib.mt_se_bwd(L.ptr(cd["da"]) if first else None, L.ptr(cd["z"]) if first else None, L.ptr(cd["scale"]) if first else None,
                          L.ptr(cd["shift"]) if first else None, L.ptr(fwd["gate"]), L.ptr(fwd["hidden"]), L.ptr(fwd["pooled"]),
                          L.ptr(cd["w1"]), L.ptr(cd["w2"]), L.ptr(o["dgate"]), L.ptr(o["dpre2"]), L.ptr(o["dhid"]), L.ptr(o["dpooled"]),
                          L.ptr(o["dw1"]), L.ptr(o["db1"]), L.ptr(o["dw2"]), L.ptr(o["db2"]), N, HW, C, CS, mask, L.ptr(scratch),
                          L.stream_ptr()), "mt_se_bwd")
    torch.cuda.synchronize()
    assert _bands_intact(xbuf) and all(_bands_intact(b[0]) for b in bufs.values()), "mt_se_bwd wrote outside its outputs"
    shapes = {"dgate": (N, C), "dpre2": (N, C), "dhid": (N, CS), "dpooled": (N, C), "dw1": (CS, C), "db1": (CS,), "dw2": (C, CS), "db2": (C,)}
    return {n: o[n].reshape(shapes[n]) for n in o}


def _se_bwd_compare(fig, tag, got, ref, N, canary):
    for name in _SE_DATA:
        for n in sorted({0, N - 1}):
            fig.close("se_bwd.data", f"{tag} {name}, image {n}", got[name][n], ref[name][n])
    for name in _SE_WGRAD:
        fig.close("se_bwd.wgrad", f"{tag} {name} (on the canary)", got[name], ref[name] + canary)


@pytest.mark.parametrize("N,HW,C,CS", SE_BWD_SHAPES)
def test_squeeze_excite_backward_vs_fp64(N, HW, C, CS):
    """mt_se_bwd with parts 3 (reduction + adjoint + weight gradients) and parts 6 (dgate given; da and z NULL) against R.se_bwd in
    fp64, the weight gradients accumulated onto their canary; deterministic mode (unsliced reduction, one weight-gradient block per
    channel group) against the same, bit-identical across two launches."""
    c = _se_inputs(N, HW, C, CS, 10 * C + CS + HW + N)
    fwd32 = [v.float() for v in _se_fwd_ref(c, F64, N, HW)]                            # the forward's outputs, rounded from fp64
    ref = _se_bwd_ref(c, fwd32, F64, N, HW)
    dgate32 = ref["dgate"].float()
    ref6 = _se_bwd_ref(c, fwd32, F64, N, HW, dgate=dgate32)
    what = f"se_bwd N{N} HW{HW} C{C} CS{CS}"
    if YARD:
        _se_bwd_compare(_Figures(what, True), "fp32", _se_bwd_ref(c, fwd32, torch.float32, N, HW), ref, N, 0.0)
    cd = {n: _d(v) for n, v in c.items()}
    fwd = {n: _d(v) for n, v in zip(("pooled", "hidden", "gate"), fwd32)}
    fig = _Figures(what)
    got = _se_bwd_launch(cd, fwd, N, HW, C, CS, 3)
    _se_bwd_compare(fig, "mt_se_bwd parts 3:", got, ref, N, CANARY)
    got6 = _se_bwd_launch(cd, fwd, N, HW, C, CS, 6, dgate_in=_d(dgate32))
    _se_bwd_compare(fig, "mt_se_bwd parts 6:", got6, ref6, N, CANARY)
    fig.true("parts 6 leaves the given dgate as it was", torch.equal(got6["dgate"].cpu(), dgate32))
    with _det(True):
        d1 = _se_bwd_launch(cd, fwd, N, HW, C, CS, 3)
        d2 = _se_bwd_launch(cd, fwd, N, HW, C, CS, 3)
    _se_bwd_compare(fig, "mt_se_bwd parts 3, deterministic:", d1, ref, N, CANARY)
    fig.true("two deterministic launches give the same bits", all(torch.equal(d1[n], d2[n]) for n in d1))
    fig.true("no NaN left in the stored outputs", not any(bool(torch.isnan(got[n]).any()) for n in _SE_DATA))
    fig.done()


def test_squeeze_excite_backward_refusals():
    lib, b = L.get(), _scratch()
    p, s = L.ptr(b), L.stream_ptr()

    def call(C, CS, mask, scratch):
        return lib.mt_se_bwd(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 2, 49, C, CS, mask, scratch, s)

    assert call(96, 49, 3, p) == MT_ERR_UNSUPPORTED
    assert call(6, 4, 3, p) == MT_ERR_ARG                 # C % 4 != 0
    assert call(96, 4, 1, None) == MT_ERR_ARG             # the reduction and the adjoint need the scratch
    assert call(96, 4, 4, None) == MT_ERR_ARG
    assert b.abs().sum().item() == 0.0


# ---- 5. mt_bn_finalize / mt_bn_bwd_finalize ----------------------------------------------------------------------------------------

def _split_over_slots(total, slots, g):
    """[|slots|][C] fp64 per-slot values that add up to about `total`; returns them and the ABI's buffer holding them (fp64, or the
    two integer limbs), plus the exact total the buffer encodes."""
    n = abs(slots)
    wts = torch.rand(n, total.shape[0], generator=g, dtype=F64) + 0.1
    per = total * wts / wts.sum(0)
    if slots > 0:
        return per, per.sum(0)
    hi = torch.trunc(per)
    lo = torch.round((per - hi) * 2.0 ** 44)
    return (hi.long(), lo.long()), (hi + lo * 2.0 ** -44).sum(0)


def _stats_fill(a, b, slots, C):
    """The device accumulator [|slots|][2][C] (x 2 limbs) holding the per-slot values a, b."""
    if slots > 0:
        return _d(torch.stack([a, b], dim=1).reshape(-1))
    limbs = torch.stack([torch.stack([a[0], b[0]], dim=1), torch.stack([a[1], b[1]], dim=1)])        # [2][n][2][C] int64
    return _d(limbs.reshape(-1)).view(F64)


@pytest.mark.parametrize("count", [1, 300])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("slots", [1, 32, -32])
@pytest.mark.parametrize("C", [24, 40, 1152])
def test_batchnorm_finalize_vs_fp64(C, slots, training, count):
    """mt_bn_finalize against R.bn_finalize in fp64 from accumulators filled on the host: scale, shift, mean, invstd and the running
    statistics after one step (untouched in eval mode); count 1 (no unbiased correction), a channel whose Q / count - m^2 comes out
    negative (clamped to 0), running_mean = NULL in training, mean_invstd = NULL."""
    g = _gen(C + slots + 7 * training + count)
    mom = 0.01
    m = torch.randn(C, generator=g, dtype=F64) + 0.5
    m[1] = 0.05                                                 # (small: the clamped channel stays well-conditioned in fp32 too)
    var = torch.rand(C, generator=g, dtype=F64) + 0.3
    S, Q = m * count, (var + m * m) * count
    Q[1] = S[1] * S[1] / count * (1 - 1e-9)                     # Q / count - m^2 = -1e-9 m^2: must be clamped
    a, S_enc = _split_over_slots(S, slots, g)
    bq, Q_enc = _split_over_slots(Q, slots, g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ref = R.bn_finalize(S_enc, Q_enc, count, *_to(F64, gamma, beta, rm, rv), EPS, mom, bool(training))
    if training:
        assert float(Q_enc[1] / count - (S_enc[1] / count) ** 2) < 0 and abs(float(ref["invstd"][1]) * EPS ** 0.5 - 1) < 1e-12
    names = ("scale", "shift", "mean", "invstd", "running_mean", "running_var")
    what = f"bn_finalize C{C} slots{slots} training{training} count{count}"
    if YARD:
        y = R.bn_finalize(S_enc.float(), Q_enc.float(), count, gamma, beta, rm, rv, EPS, mom, bool(training))
        for n in names:
            _Figures(what, True).close("bn_finalize", n, y[n], ref[n])
    st_d, gamma_d, beta_d = _stats_fill(a, bq, slots, C), _d(gamma), _d(beta)
    fig = _Figures(what)
    for with_running, with_mi in ((True, True), (False, False)):
        if not training and not with_running:
            continue
        bufs = {n: _guarded(C) for n in ("scale", "shift")}
        bufs["mi"] = _guarded(2 * C)
        rmb, rvb = _guarded(C), _guarded(C)
        rmb[1].copy_(rm); rvb[1].copy_(rv)
        L.check(L.get().mt_bn_finalize(L.ptr(st_d), slots, float(count), L.ptr(gamma_d), L.ptr(beta_d),
                                       L.ptr(rmb[1]) if with_running else None, L.ptr(rvb[1]) if with_running else None,
                                       L.ptr(bufs["scale"][1]), L.ptr(bufs["shift"][1]), L.ptr(bufs["mi"][1]) if with_mi else None, C,
                                       EPS, mom, training, L.stream_ptr()), "mt_bn_finalize")
        torch.cuda.synchronize()
        tag = "mt_bn_finalize" + ("" if with_running else ", running = NULL, mean_invstd = NULL")
        fig.true(f"{tag}: guard bands intact", all(_bands_intact(b[0]) for b in list(bufs.values()) + [rmb, rvb]))
        fig.close("bn_finalize", f"{tag} scale", bufs["scale"][1], ref["scale"])
        fig.close("bn_finalize", f"{tag} shift", bufs["shift"][1], ref["shift"])
        if with_mi:
            fig.close("bn_finalize", f"{tag} mean", bufs["mi"][1][:C], ref["mean"])
            fig.close("bn_finalize", f"{tag} invstd", bufs["mi"][1][C:], ref["invstd"])
            fig.true("the clamped channel's invstd is eps^-1/2", not training or abs(float(bufs["mi"][1][C + 1]) * EPS ** 0.5 - 1) < 1e-6)
        else:
            fig.true("mean_invstd = NULL: untouched", bool(torch.isnan(bufs["mi"][1]).all()))
        if training and with_running:
            fig.close("bn_finalize", f"{tag} running_mean", rmb[1], ref["running_mean"])
            fig.close("bn_finalize", f"{tag} running_var", rvb[1], ref["running_var"])
        else:
            fig.true(f"{tag}: the running statistics are untouched", torch.equal(rmb[1].cpu(), rm) and torch.equal(rvb[1].cpu(), rv))
    fig.done()


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("slots", [1, 32, -32])
@pytest.mark.parametrize("C", [24, 40, 1152])
def test_batchnorm_backward_finalize_vs_fp64(C, slots, training):
    """mt_bn_bwd_finalize against R.bn_bwd_finalize in fp64: kabc (kb = kc = 0 exactly in eval mode), dgamma and dbeta accumulated onto
    their canary; dgamma = dbeta = NULL."""
    g = _gen(3 * C + slots + training)
    count = 300
    S1, S2 = (torch.randn(C, generator=g, dtype=F64) * 5 + 20) , (torch.randn(C, generator=g, dtype=F64) * 5 - 15)
    a, S1_enc = _split_over_slots(S1, slots, g)
    b2, S2_enc = _split_over_slots(S2, slots, g)
    gamma = torch.rand(C, generator=g) + 0.5
    mi = torch.stack([torch.randn(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5])
    kabc, add_g, add_b = R.bn_bwd_finalize(S1_enc, S2_enc, count, gamma.double(), mi.double(), bool(training))
    what = f"bn_bwd_finalize C{C} slots{slots} training{training}"
    if YARD:
        y = R.bn_bwd_finalize(S1_enc.float(), S2_enc.float(), count, gamma, mi, bool(training))
        for i, n in enumerate(("ka", "kb", "kc")):
            _Figures(what, True).close("bn_bwd_finalize.kabc", n, y[0][i], kabc[i])
        _Figures(what, True).close("bn_bwd_finalize.grads", "dgamma", y[1], add_g)
        _Figures(what, True).close("bn_bwd_finalize.grads", "dbeta", y[2], add_b)
    st_d, gamma_d, mi_d = _stats_fill(a, b2, slots, C), _d(gamma), _d(mi)
    fig = _Figures(what)
    for with_grads in (True, False):
        kbuf, k_d = _guarded(3 * C)
        gbuf, dg = _guarded(C, CANARY)
        bbuf, db = _guarded(C, CANARY)
        L.check(L.get().mt_bn_bwd_finalize(L.ptr(st_d), slots, float(count), L.ptr(gamma_d), L.ptr(mi_d), L.ptr(k_d),
                                           L.ptr(dg) if with_grads else None, L.ptr(db) if with_grads else None, C, training,
                                           L.stream_ptr()), "mt_bn_bwd_finalize")
        torch.cuda.synchronize()
        tag = "mt_bn_bwd_finalize" + ("" if with_grads else ", dgamma = dbeta = NULL")
        fig.true(f"{tag}: guard bands intact", _bands_intact(kbuf) and _bands_intact(gbuf) and _bands_intact(bbuf))
        k_c = k_d.reshape(3, C).cpu()
        fig.close("bn_bwd_finalize.kabc", f"{tag} ka", k_c[0], kabc[0])
        if training:
            fig.close("bn_bwd_finalize.kabc", f"{tag} kb", k_c[1], kabc[1])
            fig.close("bn_bwd_finalize.kabc", f"{tag} kc", k_c[2], kabc[2])
        else:
            fig.true(f"{tag}: kb = kc = 0 in eval mode", float(k_c[1:].abs().sum()) == 0.0)
        if with_grads:
            fig.close("bn_bwd_finalize.grads", f"{tag} dgamma (on the canary)", dg, add_g + CANARY)
            fig.close("bn_bwd_finalize.grads", f"{tag} dbeta (on the canary)", db, add_b + CANARY)
        else:
            fig.true(f"{tag}: untouched", bool((dg == CANARY).all() and (db == CANARY).all()))
    fig.done()


# ---- 6. mt_bn_act_bwd / mt_bn_act_fwd ----------------------------------------------------------------------------------------------

BN_ACT_CASES = [(act, gate, rs, 258, 49, C, slots) for act in (0, 1, 2) for gate, rs in ((1, 1), (0, 0), (1, 0), (0, 1))
                for C, slots in ((24, 8), (96, -8))]                       # rows 49 * 5 + 13: no multiple of PB, the last image partial
BN_ACT_CASES += [(1, 1, 1, 3500, 49, 1152, 8), (2, 0, 1, 3500, 196, 1152, -8)]     # 700 row groups of PB 5 for a cap of 4096 / 6 = 682 blocks


@pytest.mark.parametrize("act,with_gate,with_rs,rows,hw,C,slots", BN_ACT_CASES)
def test_activation_adjoint_vs_fp64(act, with_gate, with_rs, rows, hw, C, slots):
    """mt_bn_act_bwd: du (first / last image, first / last channels) and the two sums separately against R.bn_act_bwd in fp64, with
    and without gate + dpool and rowscale; dout = NULL gives the same sums."""
    g = _gen(rows + C + 10 * act + with_gate + 2 * with_rs)
    N = -(-rows // hw)
    din = torch.randn(rows, C, generator=g) + 0.5
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.5
    z = _off_the_kink(torch.randn(rows, C, generator=g), scale, shift)
    mi = torch.stack([torch.randn(C, generator=g) * 0.5 + 1.0, torch.rand(C, generator=g) + 0.5])
    gate = torch.rand(N, C, generator=g) * 0.8 + 0.1 if with_gate else None
    dpool = torch.randn(N, C, generator=g) * hw ** 0.5 if with_gate else None
    rs = torch.where(torch.arange(N) % 3 == 1, 0.0, 1.25) if with_rs else None          # drop-connect: some images dropped
    ref = R.bn_act_bwd(*_to(F64, din, z, scale, shift, mi, gate, dpool, rs), hw, act)
    what = f"bn_act_bwd act{act} gate{with_gate} rowscale{with_rs} rows{rows} hw{hw} C{C} slots{slots}"
    last = (N - 1) * hw

    def compare(fig, tag, du, sums):
        if du is not None:
            fig.close("bn_act_bwd.du", f"{tag} du first image", du[:hw], ref[0][:hw])
            fig.close("bn_act_bwd.du", f"{tag} du last image", du[last:], ref[0][last:])
            fig.close("bn_act_bwd.du", f"{tag} du middle images", du[hw:last], ref[0][hw:last])
            fig.close("bn_act_bwd.du", f"{tag} du last 4 channels", du[:, -4:], ref[0][:, -4:])
        _sums(fig, "bn_act_bwd.sums", f"{tag} sum du", sums[0], ref[1], 4)
        _sums(fig, "bn_act_bwd.sums", f"{tag} sum du xhat", sums[1], ref[2], 4)

    if YARD:
        y = R.bn_act_bwd(din, z, scale, shift, mi, gate, dpool, rs, hw, act)
        compare(_Figures(what, True), "fp32", y[0], torch.stack(y[1:]))
    dv = [None if t is None else _d(t) for t in (din, z, scale, shift, mi, gate, dpool, rs)]
    fig = _Figures(what)
    for with_out in (True, False):
        obuf, du = _guarded(rows * C)
        sbuf, st = _stats_buffer(slots, C)
        L.check(L.get().mt_bn_act_bwd(*[L.ptr(t) for t in dv], L.ptr(du) if with_out else None, L.ptr(st), slots, rows, C, hw, act,
                                      L.stream_ptr()), "mt_bn_act_bwd")
        torch.cuda.synchronize()
        fig.true("guard bands intact", _bands_intact(obuf) and _bands_intact(sbuf))
        compare(fig, "mt_bn_act_bwd" + ("" if with_out else ", dout = NULL:"), du.reshape(rows, C) if with_out else None, _stats_read(st, slots, C))
        if not with_out:
            fig.true("dout = NULL: nothing stored", bool(torch.isnan(du).all()))
    fig.done()


@pytest.mark.parametrize("act,with_res,with_rs,rows,C", [(1, 0, 0, 3300, 1280), (0, 1, 1, 258, 24), (2, 0, 0, 258, 40)])
def test_activation_forward_vs_fp64(act, with_res, with_rs, rows, C):
    """mt_bn_act_fwd against R.bn_act_fwd in fp64; rows 3300 x C 1280 = 4125 blocks' worth for a cap of 4096: the grid-stride loop runs."""
    g = _gen(rows + C)
    hw = 49
    N = -(-rows // hw)
    z = torch.randn(rows, C, generator=g)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    res = torch.randn(rows, C, generator=g) if with_res else None
    rs = torch.where(torch.arange(N) % 3 == 1, 0.0, 1.25) if with_rs else None
    ref = R.bn_act_fwd(*_to(F64, z, scale, shift, res), act, None if rs is None else rs.double(), hw)
    what = f"bn_act_fwd act{act} res{with_res} rowscale{with_rs} rows{rows} C{C}"
    if YARD:
        _Figures(what, True).close("bn_act_fwd", "y", R.bn_act_fwd(z, scale, shift, res, act, rs, hw), ref)
    fig = _Figures(what)
    obuf, y = _guarded(rows * C)
    dv = [None if t is None else _d(t) for t in (z, scale, shift, res, rs)]
    L.check(L.get().mt_bn_act_fwd(L.ptr(dv[0]), L.ptr(dv[1]), L.ptr(dv[2]), L.ptr(dv[3]), L.ptr(y), rows, C, act, L.ptr(dv[4]), hw,
                                  L.stream_ptr()), "mt_bn_act_fwd")
    torch.cuda.synchronize()
    fig.true("guard bands intact", _bands_intact(obuf))
    y = y.reshape(rows, C)
    half = rows // 2
    fig.close("bn_act_fwd", "mt_bn_act_fwd y, first half of the rows", y[:half], ref[:half])
    fig.close("bn_act_fwd", "mt_bn_act_fwd y, second half (past the block cap)", y[half:], ref[half:])
    fig.close("bn_act_fwd", "mt_bn_act_fwd y, last 4 channels", y[:, -4:], ref[:, -4:])
    fig.done()


# ---- 7. mt_stem_conv_wgrad ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,u8,det", [(H, W, u8, False) for H, W in ((8, 12), (9, 13), (6, 224), (6, 258)) for u8 in (0, 1)]
                         + [(8, 12, 0, True), (8, 12, 1, True)])
def test_stem_weight_gradient_vs_fp64(H, W, u8, det):
    """mt_stem_conv_wgrad (TF-SAME) accumulated onto its canary against R.stem_wgrad in fp64, per kernel row (the padded taps are
    kh = 0 / kw = 0 at odd sizes, kh = 2 / kw = 2 at even ones).  Default mode: the MFMA kernel up to Wo 128, the outer-product kernel
    at W 258; deterministic mode (8 x 12 again): the outer-product kernel, bit-identical across two launches."""
    N = 2
    g = _gen(H + W + u8)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8) if u8 else torch.randn(N, H, W, 3, generator=g) + 0.5
    du = torch.randn(N * Ho * Wo, 32, generator=g) + 0.5
    z = torch.randn(N * Ho * Wo, 32, generator=g)
    kabc = torch.stack([torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1, torch.randn(32, generator=g) * 0.1])
    ref = R.stem_wgrad(*_to(F64, du, z, kabc, x), N, H, W)
    what = f"stem_wgrad {H}x{W} u8={u8} det={det}"

    def compare(fig, tag, dw, canary):
        for kh in range(3):
            fig.close("stem_wgrad", f"{tag} dw[:, :, {kh}, :]", dw[:, :, kh], ref[:, :, kh] + canary)
        for kw in (0, 2):
            fig.close("stem_wgrad", f"{tag} dw[:, :, :, {kw}]", dw[..., kw], ref[..., kw] + canary)

    if YARD:
        compare(_Figures(what, True), "fp32", R.stem_wgrad(du, z, kabc, x.float(), N, H, W), 0.0)
    dv = [_d(t) for t in (du, z, kabc, x)]
    fig = _Figures(what)
    got = []
    with _det(det):
        for _ in range(2 if det else 1):
            wbuf, dw = _guarded(32 * 27, CANARY)
            L.check(L.get().mt_stem_conv_wgrad(L.ptr(dv[0]), L.ptr(dv[1]), L.ptr(dv[2]), L.ptr(dv[3]), u8, L.ptr(dw), N, H, W, L.stream_ptr()),
                    "mt_stem_conv_wgrad")
            torch.cuda.synchronize()
            fig.true("guard bands intact", _bands_intact(wbuf))
            got.append(dw.reshape(32, 3, 3, 3))
    compare(fig, "mt_stem_conv_wgrad", got[0], CANARY)
    if det:
        fig.true("two deterministic launches give the same bits", torch.equal(got[0], got[1]))
    fig.done()


def test_stem_weight_gradient_refusals():
    """Host-side checks only: H and W of different parity need different leading pads, which mt_stem_conv_fwd refuses too."""
    lib, b = L.get(), _scratch()
    p, s = L.ptr(b), L.stream_ptr()
    assert lib.mt_stem_conv_wgrad(p, p, p, p, 0, p, 1, 9, 12, s) == MT_ERR_UNSUPPORTED
    assert lib.mt_stem_conv_wgrad(p, p, p, p, 1, p, 1, 8, 13, s) == MT_ERR_UNSUPPORTED
    assert lib.mt_stem_conv_wgrad(p, p, p, None, 0, p, 1, 8, 12, s) == MT_ERR_ARG
    assert b.abs().sum().item() == 0.0


# ---- 8. mt_conv_weight_unpack_grad -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Co,Ci,k,ld", [(32, 3, 3, 28), (64, 32, 3, 288)])
def test_weight_unpack_inverts_pack(Co, Ci, k, ld):
    """mt_conv_weight_pack(transpose = 0) is R.conv_weight_pack exactly; mt_conv_weight_unpack_grad of it (dw += ...: onto zeros) gives
    the weights back exactly, whatever the padding columns hold."""
    w = torch.randn(Co, Ci, k, k, generator=_gen(Co))
    lib = L.get()
    pbuf, wp = _guarded(Co * ld)
    w_d = _d(w)
    L.check(lib.mt_conv_weight_pack(L.ptr(w_d), L.ptr(wp), Co, Ci, k, ld, 0, L.stream_ptr()), "mt_conv_weight_pack")
    torch.cuda.synchronize()
    assert _bands_intact(pbuf)
    assert torch.equal(wp.reshape(Co, ld).cpu(), R.conv_weight_pack(w, ld))
    wp.reshape(Co, ld)[:, k * k * Ci:] = float("nan")                      # the padding columns are not read
    ubuf, dw = _guarded(Co * Ci * k * k, 0.0)
    L.check(lib.mt_conv_weight_unpack_grad(L.ptr(wp), L.ptr(dw), Co, Ci, k, ld, L.stream_ptr()), "mt_conv_weight_unpack_grad")
    torch.cuda.synchronize()
    assert _bands_intact(ubuf)
    assert torch.equal(dw.reshape(Co, Ci, k, k).cpu(), w)
    assert torch.equal(R.conv_weight_unpack(R.conv_weight_pack(w, ld), Co, Ci, k), w)
    L.check(lib.mt_conv_weight_unpack_grad(L.ptr(wp), L.ptr(dw), Co, Ci, k, ld, L.stream_ptr()), "mt_conv_weight_unpack_grad")
    torch.cuda.synchronize()
    assert torch.equal(dw.reshape(Co, Ci, k, k).cpu(), w + w)                # it accumulates
