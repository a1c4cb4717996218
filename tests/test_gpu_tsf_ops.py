"""Per-kernel parity of the Size-Invariant TimeSformer's hand-written non-GEMM kernels (csrc/tsf_fwd.hip, csrc/tsf_bwd.hip: LayerNorm,
the embeddings, the divided-attention core, the head, the column sums, the attention aggregation) against plain fp64 torch on the CPU:
the operation's definition or autograd of it (tests/tsf_ref.py for the attention core).  Every test calls the C ABI directly on
buffers pre-filled with NaN or a canary, at shapes picked for the kernels' tails and dispatch thresholds rather than the workload's,
and compares per SECTION (cls rows / patch rows / each of dq, dk, dv ...): one small-magnitude slice cannot hide behind the largest
value of a whole tensor.  The exact checks (canaries, zeros, refusals, plane-vs-fp32 equality, run-to-run identity) have no tolerance;
every other gate is twice the worst case measured on an MI355X, rounded up to one significant digit (the measured value, its case and
the error of the same reference evaluated in fp32 torch on the CPU -- the yardstick -- are next to the gate).  MT_TEST_YARDSTICK=1
prints the yardstick figures beside the kernels'."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from mintime_amd import lib as L

from . import tsf_ref as R
from .util import GRAD_TOL_UNIT, rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

CANARY = 7.0
GUARD_BITS = -2 ** 31          # the guard bands hold -0.0: any store shows, and so does a read-modify-write that adds +0.0
EPS = 1e-5
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3          # csrc/common.hpp
YARD = bool(os.environ.get("MT_TEST_YARDSTICK"))
n = 49
DH = 64
SCALE = DH ** -0.5

# gate = 2 x the worst case measured on an MI355X over every comparison that uses it, one significant digit up.  Beside it: that worst
# case, and the yardstick -- the largest error of the same reference evaluated in fp32 torch on the CPU against fp64, same cases.
ATTN_FWD_TOL = {"moderate": 9e-7,          # 4.2e-7 (out patch rows, B 2 H 8 F 8, all-ones mask, space); yardstick 9.8e-7
                "peaky": 5e-6,             # 2.5e-6 (out patch rows, B 3 H 2 F 8, all-ones mask, space); yardstick 3.4e-6
                "negative": 2e-5}          # 8.5e-6 (out patch rows, B 1 H 1 F 8, random ident, space); yardstick 1.7e-5
ATTN_BWD_TOL = {"moderate": 9e-7,          # 4.2e-7 (dv patch rows, B 3 H 2 F 8, random ident, space); yardstick 1.4e-6
                "peaky": 7e-6,             # 3.0e-6 (dq patch rows, B 3 H 2 F 8, random ident, space); yardstick 4.3e-6
                "negative": 9e-5}          # 4.3e-5 (dk cls rows of the plane output, B 1 H 1 F 8, zero-mask clip, space); yardstick 8.6e-5
LN_FWD_TOL = 3e-7                          # 1.4e-7 (y, dim 516, 393 rows); yardstick 1.5e-7
LN_FWD_OFFSET_TOL = 5e-5                   # y of the row with mean 1e3, standard deviation 1: 2.1e-5 (dim 64); yardstick 1.9e-5
LN_BWD_DX_TOL = 4e-7                       # 1.6e-7 (fused kernel, dim 64, 7 rows); yardstick 1.3e-7
LN_BWD_SUMS_TOL = 9e-7                     # 4.2e-7 (dbeta of the cols kernel, dim 64, 393 rows, skip 393); yardstick 1.9e-7
HEAD_FWD_TOL = 6e-7                        # 2.7e-7 (logits, dim 512, 3 classes, B 1); yardstick 8.0e-7
HEAD_BWD_TOL = 4e-6                        # 2.0e-6 (dbeta, dim 512, 1 class, B 2); yardstick 1.9e-6.  Both are the rounding of the
#                                            accumulation onto the O(1) starting value, measured against a gradient of size ~0.1
EMBED_FWD_TOL = 2e-7                       # 8.7e-8 (patch rows, B 3 F 16 dim 320, positions = NULL); yardstick 8.7e-8
EMBED_BWD_TOL = 1e-6                       # 4.9e-7 (dpos_emb, B 3 F 16 dim 320, frame-number positions); yardstick 6.0e-7
COLSUM_TOL = 8e-7                          # 3.9e-7 (M 1000 N 1, deterministic mode); yardstick 1.2e-6
AGG_TOL = {1: 6e-7,                        # 2.6e-7 (time row, F 32, BH 24); yardstick 1.6e-7
           50000: 4e-5}                    # 1.6e-5 (combined row, F 8, BH 1); yardstick 2.7e-6: fp32 rounding of chunk means of ~127,
#                                            whose differences the softmax exponentiates
assert max(max(ATTN_FWD_TOL.values()), max(ATTN_BWD_TOL.values()), LN_FWD_OFFSET_TOL, LN_BWD_DX_TOL, LN_BWD_SUMS_TOL, HEAD_BWD_TOL,
           EMBED_BWD_TOL, COLSUM_TOL, max(AGG_TOL.values())) <= GRAD_TOL_UNIT
assert max(ATTN_FWD_TOL["moderate"], LN_FWD_TOL, HEAD_FWD_TOL, EMBED_FWD_TOL, AGG_TOL[1]) <= 1e-5


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
    """A device buffer of `numel` elements holding `fill`, between two 64-element guard bands (an over-run shows in the bands)."""
    buf = torch.full((numel + 128,), -0.0, dtype=dtype, device=dev)
    body = buf[64:64 + numel]
    body.fill_(fill)
    return buf, body


def _bands_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[:64] == GUARD_BITS).all() and (bits[-64:] == GUARD_BITS).all())


class _Figures:
    """Collects the figures of one test, prints each before anything is asserted, then fails on all that missed."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def close(self, name, got, ref, tol):
        e = rel_err(got, ref)
        print(f"FIG {self.what} | {name} | {e:.3e} | tol {tol:.0e}")
        if not e <= tol:
            self.bad.append(f"{name}: {e:.3e} > {tol:.0e}")
        return e

    def yard(self, name, got32, ref):
        print(f"YARD {self.what} | {name} | {rel_err(got32, ref):.3e}")

    def true(self, name, cond):
        if not bool(cond):
            print(f"FIG {self.what} | {name} | FALSE")
            self.bad.append(name)

    def done(self):
        assert not self.bad, f"{self.what}: " + "; ".join(self.bad)


# ---- 1. the divided-attention core ---------------------------------------------------------------------------------------------

ATTN_SHAPES = [(1, 1, 8),      # 49 time wavefronts at 4 per block: a 1-of-4 tail; factored scratch R = 7
               (3, 2, 8),      # 294 wavefronts: a 2-of-4 tail
               (1, 3, 16),     # 147 wavefronts at 2 per block: an odd tail; R = 5
               (1, 1, 32),     # the older launch_patch* templates: 25 chunks with tails forward and backward, a last chunk of one patch
               (2, 8, 8)]      # the model's own form
ATTN_MASKS = ["ones", "ragged", "random", "zeroclip"]
ATTN_REGIMES = ["moderate", "peaky", "negative"]
_BLOCKS = {8: [3, 3, 2], 16: [7, 5, 4], 32: [14, 10, 8]}


def _block_ident(B, F):
    ident = torch.zeros(B, F, F, dtype=torch.bool)
    o = 0
    for k in _BLOCKS[F]:
        ident[:, o:o + k, o:o + k] = True
        o += k
    return ident


def _attn_masks(kind, B, F, g):
    """(mask [B, F] bool, ident [B, F, F] bool, index of the clip whose mask is all zero or None)."""
    mask = torch.ones(B, F, dtype=torch.bool)
    ident = torch.ones(B, F, F, dtype=torch.bool)
    zero_clip = None
    if kind == "ragged":
        ident = _block_ident(B, F)
        mask[:, F - max(1, _BLOCKS[F][-1] // 2):] = False            # the last frames of the last identity are padding
    elif kind == "random":
        ident = torch.rand(B, F, F, generator=g) < 0.5
        assert all(not torch.equal(ident[b], ident[b].t()) for b in range(B))
        mask[:, 1] = False
    elif kind == "zeroclip":
        ident = _block_ident(B, F)
        zero_clip = B - 1
        mask[zero_clip] = False
    return mask, ident, zero_clip


def _attn_qkv(regime, B, N, H, g):
    inner = H * DH
    qkv = torch.randn(B, N, 3 * inner, generator=g) * 0.5
    if regime == "peaky":              # q . k * scale has standard deviation 0.125 * 8 * sigma^2 = 8
        qkv[..., :2 * inner] *= 2.0 * (8.0 ** 0.5)
    elif regime == "negative":         # q = +a u, k = -a u (+ noise): every score, the cls key's included, is near -a^2 * scale = -40
        u = Fn.normalize(torch.randn(H, DH, generator=g), dim=1).reshape(inner)
        a = (40.0 / SCALE) ** 0.5
        noise = torch.randn(B, N, 2 * inner, generator=g) * 0.05
        qkv[..., :inner] = a * u + noise[..., :inner]
        qkv[..., inner:2 * inner] = -a * u + noise[..., inner:]
    return qkv


def _attn_case(B, H, F, kind, regime, seed=0):
    g = _gen(1000 * B + 100 * H + F + seed)
    N = 1 + F * n
    mask, ident, zero_clip = _attn_masks(kind, B, F, g)
    qkv = _attn_qkv(regime, B, N, H, g)
    dout = torch.randn(B, N, H * DH, generator=g)
    return qkv, dout, mask, ident, zero_clip


def _attn_fwd(qkv_d, mask_d, ident_d, B, H, F, mode, fill=float("nan"), fp32=True, att=True, planes=False):
    N, inner = 1 + F * n, H * DH
    obuf, o = _guarded(B * N * inner, fill) if fp32 else (None, None)
    abuf, a = _guarded(B * H * N) if att else (None, None)
    op = None
    if planes:
        op = L.planes_empty(B * N, inner, dev)
        op.fill_(float("nan"))
    L.check(L.get().mt_attn_fwd(L.ptr(qkv_d), L.ptr(o), L.ptr(a), L.ptr(mask_d), L.ptr(ident_d), B, H, F, n, mode, SCALE, L.ptr(op),
                                L.stream_ptr()), "mt_attn_fwd")
    torch.cuda.synchronize()
    assert (obuf is None or _bands_intact(obuf)) and (abuf is None or _bands_intact(abuf)), "mt_attn_fwd wrote outside its outputs"
    return (o.reshape(B, N, inner) if fp32 else None), (a.reshape(B * H, N) if att else None), op


def _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode, fill=float("nan"), planes=False):
    N, inner = 1 + F * n, H * DH
    buf, dqkv = _guarded(B * N * 3 * inner, fill)
    dp = None
    if planes:
        dp = L.planes_empty(B * N, 3 * inner, dev)
        dp.fill_(float("nan"))
    L.check(L.get().mt_attn_bwd(L.ptr(qkv_d), L.ptr(dout_d), L.ptr(dqkv), L.ptr(mask_d), L.ptr(ident_d), B, H, F, n, mode, SCALE,
                                L.ptr(dp), L.stream_ptr()), "mt_attn_bwd")
    torch.cuda.synchronize()
    assert _bands_intact(buf), "mt_attn_bwd wrote outside dqkv"
    return dqkv.reshape(B, N, 3 * inner), dp


def _out_sections(fig, tag, got, ref, tol):
    fig.close(f"{tag} cls rows", got[:, 0], ref[:, 0], tol)
    fig.close(f"{tag} patch rows", got[:, 1:], ref[:, 1:], tol)


def _grad_sections(fig, tag, got, ref, tol, yard=False):
    for name, gt, rf in zip(("dq", "dk", "dv"), got.chunk(3, dim=-1), ref.chunk(3, dim=-1)):
        for rows, sl in (("cls rows", slice(0, 1)), ("patch rows", slice(1, None))):
            if yard:
                fig.yard(f"{tag} {name} {rows}", gt[:, sl], rf[:, sl])
            else:
                fig.close(f"{tag} {name} {rows}", gt[:, sl], rf[:, sl], tol)


def _planes_padding_is_zero(planes, rows, cols):
    full = L.planes_to_float(planes, planes.shape[1] * 32, cols)
    return not bool(torch.isnan(planes.float()).any()) and float(full[rows:].abs().sum()) == 0.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("regime", ATTN_REGIMES)
@pytest.mark.parametrize("kind", ATTN_MASKS)
@pytest.mark.parametrize("B,H,F", ATTN_SHAPES)
def test_attention_forward_vs_fp64(B, H, F, kind, regime, mode):
    """out (cls rows, patch rows) and cls_att of mt_attn_fwd against tests/tsf_ref.py in fp64; masked keys get exactly zero attention,
    a clip whose mask is all zero an exactly one-hot cls_att; the plane output is the exact split of the fp32 output."""
    N, inner = 1 + F * n, H * DH
    qkv, _, mask, ident, zero_clip = _attn_case(B, H, F, kind, regime)
    ref, ref_att = R.attn_ref(qkv.double(), mask, ident, H, F, n, mode, SCALE)
    qkv_d, mask_d, ident_d = _d(qkv), _d(mask.to(torch.uint8)), _d(ident.to(torch.uint8))
    out, att, _ = _attn_fwd(qkv_d, mask_d, ident_d, B, H, F, mode)
    fig = _Figures(f"attn_fwd {regime} B{B} H{H} F{F} {kind} mode{mode}")
    tol = ATTN_FWD_TOL[regime]
    _out_sections(fig, "out", out, ref, tol)
    fig.close("cls_att", att, ref_att, tol)
    if YARD:
        r32, a32 = R.attn_ref(qkv, mask, ident, H, F, n, mode, SCALE)
        fig.yard("out cls rows", r32[:, 0], ref[:, 0])
        fig.yard("out patch rows", r32[:, 1:], ref[:, 1:])
        fig.yard("cls_att", a32, ref_att)
    att_c = att.cpu()
    keep = torch.cat((torch.ones(B, 1, dtype=torch.bool), mask.repeat_interleave(n, dim=1)), dim=1).repeat_interleave(H, dim=0)
    fig.true("masked keys are exactly 0 in cls_att", (att_c[~keep] == 0).all())
    rowsum = float((att_c.double().sum(1) - 1.0).abs().max())
    print(f"FIG {fig.what} | cls_att row sums - 1 | {rowsum:.3e} | tol {tol:.0e}")
    fig.true("cls_att rows sum to 1", rowsum <= tol)
    if zero_clip is not None:
        z = att_c[zero_clip * H:(zero_clip + 1) * H]
        fig.true("all-zero mask: cls_att is exactly one-hot", bool((z[:, 0] == 1).all() and (z[:, 1:] == 0).all()))
    # plane output: alone (out = NULL) and together with the fp32 output
    _, _, op = _attn_fwd(qkv_d, mask_d, ident_d, B, H, F, mode, fp32=False, att=False, planes=True)
    fig.true("planes == split of the fp32 output", torch.equal(L.planes_to_float(op, B * N, inner), out.reshape(B * N, inner)))
    fig.true("plane padding rows are zero", _planes_padding_is_zero(op, B * N, inner))
    _out_sections(fig, "planes", L.planes_to_float(op, B * N, inner).reshape(B, N, inner), ref, tol)
    out2, _, op2 = _attn_fwd(qkv_d, mask_d, ident_d, B, H, F, mode, att=False, planes=True)
    fig.true("fp32 + planes in one call: same values", torch.equal(out2, out) and torch.equal(op2, op))
    fig.done()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("regime", ATTN_REGIMES)
@pytest.mark.parametrize("kind", ATTN_MASKS)
@pytest.mark.parametrize("B,H,F", ATTN_SHAPES)
def test_attention_backward_vs_fp64(B, H, F, kind, regime, mode):
    """dq, dk, dv of mt_attn_bwd on cls rows and on patch rows against autograd of tests/tsf_ref.py in fp64: default mode,
    deterministic mode (twice: bit-identical), and the plane output (the factored cls hand-over at R = ceil(N / inner) scratch rows)."""
    N, inner = 1 + F * n, H * DH
    qkv, dout, mask, ident, zero_clip = _attn_case(B, H, F, kind, regime)
    ref = R.attn_bwd_ref(qkv.double(), dout.double(), mask, ident, H, F, n, mode, SCALE)
    qkv_d, dout_d, mask_d, ident_d = _d(qkv), _d(dout), _d(mask.to(torch.uint8)), _d(ident.to(torch.uint8))
    fig = _Figures(f"attn_bwd {regime} B{B} H{H} F{F} {kind} mode{mode}")
    tol = ATTN_BWD_TOL[regime]
    if YARD:
        _grad_sections(fig, "fp32", R.attn_bwd_ref(qkv, dout, mask, ident, H, F, n, mode, SCALE), ref, tol, yard=True)
    with _det(False):
        got, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode)
        _grad_sections(fig, "default", got, ref, tol)
        _, dp = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode, planes=True)
        gp = L.planes_to_float(dp, B * N, 3 * inner).reshape(B, N, 3 * inner)
        _grad_sections(fig, "planes", gp, ref, tol)
        fig.true("plane padding rows are zero", _planes_padding_is_zero(dp, B * N, 3 * inner))
        fig.true("planes: patch rows have one owner, same values as fp32", torch.equal(gp[:, 1:], got[:, 1:]))
    with _det(True):
        d1, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode)
        d2, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode)
        _grad_sections(fig, "deterministic", d1, ref, tol)
        fig.true("deterministic mode: second run bit-identical", torch.equal(d1, d2))
        _, p1 = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode, planes=True)
        _, p2 = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, mode, planes=True)
        _grad_sections(fig, "deterministic planes", L.planes_to_float(p1, B * N, 3 * inner).reshape(B, N, 3 * inner), ref, tol)
        fig.true("deterministic mode: plane output bit-identical", torch.equal(p1, p2))
    if zero_clip is not None and mode == 0:
        for tag, t in (("default", got), ("planes", gp), ("deterministic", d1)):
            fig.true(f"all-zero mask, time mode ({tag}): dk / dv of the clip's patch keys are exactly 0",
                     (t[zero_clip, 1:, inner:] == 0).all())
    fig.done()


@pytest.mark.parametrize("kind", ["ragged", "zeroclip"])
@pytest.mark.parametrize("B,H,F", ATTN_SHAPES)
def test_attention_mode2_is_the_cls_query_alone(B, H, F, kind):
    """Mode 2, forward: only row 0 of each clip is written.  Backward: dk / dv of every key and dq of row 0 are the gradient of a loss
    on row 0; the dq section of the patch rows is not written (mt_attn_bwd's header comment says so) and keeps what it held."""
    N, inner = 1 + F * n, H * DH
    qkv, dout, mask, ident, _ = _attn_case(B, H, F, kind, "moderate", seed=7)
    ref, ref_att = R.attn_ref(qkv.double(), mask, ident, H, F, n, 2, SCALE)
    dref = R.attn_bwd_ref(qkv.double(), dout.double(), mask, ident, H, F, n, 2, SCALE)
    qkv_d, dout_d, mask_d, ident_d = _d(qkv), _d(dout), _d(mask.to(torch.uint8)), _d(ident.to(torch.uint8))
    fig = _Figures(f"attn_mode2 moderate B{B} H{H} F{F} {kind}")
    out, att, _ = _attn_fwd(qkv_d, mask_d, ident_d, B, H, F, 2, fill=CANARY)
    fig.close("out cls rows", out[:, 0], ref[:, 0], ATTN_FWD_TOL["moderate"])
    fig.close("cls_att", att, ref_att, ATTN_FWD_TOL["moderate"])
    fig.true("forward: patch rows keep the canary", (out[:, 1:] == CANARY).all())
    # without mask / ident pointers: mode 2 needs neither when nothing is padded
    if kind == "ragged":
        ref1, _ = R.attn_ref(qkv.double(), torch.ones_like(mask), ident, H, F, n, 2, SCALE)
        o1, _, _ = _attn_fwd(qkv_d, None, None, B, H, F, 2, fill=CANARY)
        fig.close("out cls rows (mask = NULL)", o1[:, 0], ref1[:, 0], ATTN_FWD_TOL["moderate"])
    for det in (False, True):
        with _det(det):
            got, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, B, H, F, 2, fill=CANARY)
        tag = "deterministic" if det else "default"
        gq, gk, gv = got.chunk(3, dim=-1)
        rq, rk, rv = dref.chunk(3, dim=-1)
        fig.close(f"{tag} dq cls rows", gq[:, 0], rq[:, 0], ATTN_BWD_TOL["moderate"])
        for name, gt, rf in (("dk", gk, rk), ("dv", gv, rv)):
            fig.close(f"{tag} {name} cls rows", gt[:, 0], rf[:, 0], ATTN_BWD_TOL["moderate"])
            fig.close(f"{tag} {name} patch rows", gt[:, 1:], rf[:, 1:], ATTN_BWD_TOL["moderate"])
        fig.true(f"backward ({tag}): the dq section of the patch rows keeps the canary", (gq[:, 1:] == CANARY).all())
    # plane output is refused in mode 2, before anything is launched
    op = L.planes_empty(B * N, inner, dev)
    obuf, o = _guarded(B * N * inner, CANARY)
    rc = L.get().mt_attn_fwd(L.ptr(qkv_d), L.ptr(o), None, L.ptr(mask_d), L.ptr(ident_d), B, H, F, n, 2, SCALE, L.ptr(op), L.stream_ptr())
    torch.cuda.synchronize()
    fig.true("mode 2 with plane output is refused and writes nothing", rc == MT_ERR_ARG and bool((o == CANARY).all()))
    fig.done()


# ---- 2. LayerNorm forward ----------------------------------------------------------------------------------------------------------

def _ln_fwd(x_d, gamma_d, beta_d, rows, D, fp32=True, stats=True, planes=False):
    ybuf, y = _guarded(rows * D) if fp32 else (None, None)
    sbuf, st = _guarded(rows * 2) if stats else (None, None)
    yp = None
    if planes:
        yp = L.planes_empty(rows, D, dev)
        yp.fill_(float("nan"))
    rc = L.get().mt_layernorm_fwd(L.ptr(x_d), L.ptr(gamma_d), L.ptr(beta_d), L.ptr(y), L.ptr(st), rows, D, EPS, L.ptr(yp), L.stream_ptr())
    torch.cuda.synchronize()
    assert (ybuf is None or _bands_intact(ybuf)) and (sbuf is None or _bands_intact(sbuf)), "mt_layernorm_fwd wrote outside its outputs"
    return rc, (y.reshape(rows, D) if fp32 else None), (st.reshape(rows, 2) if stats else None), yp


@pytest.mark.parametrize("rows", [1, 5, 393])
@pytest.mark.parametrize("D", [64, 512, 516, 1024])
def test_layernorm_forward_vs_fp64(D, rows):
    """y, stats = (mean, rstd) and the plane output of mt_layernorm_fwd; a constant row (0.75: every partial sum of it is exact in fp32
    whatever the order, so the mean is exact, y == beta to the bit and rstd = 1 / sqrt(eps)) and a row with mean 1e3 and standard
    deviation 1 (a one-pass E[x^2] - mean^2 variance would lose it) sit among the ordinary rows when there are 5 or more."""
    g = _gen(D + rows)
    x = torch.randn(rows, D, generator=g) * 1.5 + 0.3
    const_row, off_row = (1, 2) if rows >= 5 else (None, None)
    if rows >= 5:
        x[const_row] = 0.75
        x[off_row] = 1000.0 + torch.randn(D, generator=g)
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.3
    xd = x.double()                                        # the reference starts from the fp32-rounded input
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    ref = (xd - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    ordinary = torch.ones(rows, dtype=torch.bool)
    if rows >= 5:
        ordinary[[const_row, off_row]] = False
    x_d, gamma_d, beta_d = _d(x), _d(gamma), _d(beta)
    fig = _Figures(f"ln_fwd D{D} rows{rows}")
    rc, y, st, _ = _ln_fwd(x_d, gamma_d, beta_d, rows, D)
    L.check(rc, "mt_layernorm_fwd")
    fig.close("y", y[ordinary], ref[ordinary], LN_FWD_TOL)
    fig.close("mean", st[ordinary, 0], mean[ordinary], LN_FWD_TOL)
    fig.close("rstd", st[ordinary, 1], rstd[ordinary], LN_FWD_TOL)
    if YARD:
        y32 = Fn.layer_norm(x, (D,), gamma, beta, EPS)
        fig.yard("y", y32[ordinary], ref[ordinary])
    if rows >= 5:
        fig.true("constant row: y == beta exactly", torch.equal(y[const_row].cpu(), beta))
        fig.true("constant row: mean exact", float(st[const_row, 0]) == 0.75)
        fig.close("constant row: rstd = 1 / sqrt(eps)", st[const_row, 1], torch.tensor(EPS, dtype=torch.float64) ** -0.5, LN_FWD_TOL)
        fig.close("offset row: y", y[off_row], ref[off_row], LN_FWD_OFFSET_TOL)
        fig.close("offset row: mean", st[off_row, 0], mean[off_row], LN_FWD_TOL)
        fig.close("offset row: rstd", st[off_row, 1], rstd[off_row], LN_FWD_TOL)
        if YARD:
            fig.yard("offset row: y", y32[off_row], ref[off_row])
    # stats are optional
    rc, y_ns, _, _ = _ln_fwd(x_d, gamma_d, beta_d, rows, D, stats=False)
    fig.true("stats = NULL: same y", rc == 0 and torch.equal(y_ns, y))
    # plane output: refused unless dim % 16 == 0; otherwise exactly the converter's split of y, padding rows zeroed
    rc, y_p, _, yp = _ln_fwd(x_d, gamma_d, beta_d, rows, D, planes=True)
    if D % 16:
        fig.true("dim % 16 != 0: plane output refused, nothing written",
                 rc == MT_ERR_ARG and bool(torch.isnan(y_p).all()) and bool(torch.isnan(yp.float()).all()))
    else:
        want = L.split_planes_blk(y, rows, D)
        fig.true("y + planes: planes == split_planes_blk(y), padding included", rc == 0 and torch.equal(yp, want) and torch.equal(y_p, y))
        rc, _, _, yp2 = _ln_fwd(x_d, gamma_d, beta_d, rows, D, fp32=False, planes=True)
        fig.true("y = NULL: planes only, same planes", rc == 0 and torch.equal(yp2, want))
        fig.true("plane padding rows are zero", _planes_padding_is_zero(yp2, rows, D))
    fig.done()


def test_layernorm_forward_refusals():
    x, gm = torch.ones(4, 1028, device=dev), torch.ones(1028, device=dev)
    buf, y = _guarded(4 * 1028, CANARY)
    lib = L.get()
    for D in (1028, 6, 0):
        assert lib.mt_layernorm_fwd(L.ptr(x), L.ptr(gm), L.ptr(gm), L.ptr(y), None, 4, D, EPS, None, L.stream_ptr()) == MT_ERR_ARG
    assert lib.mt_layernorm_fwd(L.ptr(x), L.ptr(gm), L.ptr(gm), None, None, 4, 64, EPS, None, L.stream_ptr()) == MT_ERR_ARG
    torch.cuda.synchronize()
    assert bool((y == CANARY).all()) and _bands_intact(buf)


# ---- 3. the LayerNorm backward family ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("skip", [0, 393])
@pytest.mark.parametrize("rows", [7, 393])
@pytest.mark.parametrize("D", [64, 1024])
def test_layernorm_backward_family_vs_fp64(D, rows, skip, det):
    """mt_layernorm_bwd (in place and out of place), _rows + _cols, _rows_sums + _cols_reduce at the narrowest and the widest row
    (the <4> / kernel4 instantiations at 1024; _rows_sums refuses more than 512): dx, dgamma, dbeta and the column sums of the updated
    dx with row % skip == 0 left out, accumulated onto non-zero targets; dx_planes are the exact split of the fp32 dx."""
    lib = L.get()
    g = _gen(D + rows + skip)
    x, dy, dx0 = torch.randn(rows, D, generator=g) * 1.3 + 0.2, torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    gamma = torch.rand(D, generator=g) + 0.5
    start = torch.randn(3, D, generator=g)                      # non-zero starting values of dgamma, dbeta, dx_colsum
    xd = x.double().requires_grad_(True)
    (Fn.layer_norm(xd, (D,), gamma.double(), None, EPS) * dy.double()).sum().backward()
    dx_ref = dx0.double() + xd.grad
    keep = torch.ones(rows, dtype=torch.bool)
    if skip:
        keep[::skip] = False
    mean, var = x.double().mean(1), x.double().var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (x.double() - mean[:, None]) * rstd[:, None]
    sums_ref = {"dgamma": (dy.double() * xh).sum(0), "dbeta": dy.double().sum(0), "dx_colsum": dx_ref[keep].sum(0)}
    stats = _d(torch.stack([mean, rstd], 1).float())
    dy_d, x_d, gamma_d, dx0_d = _d(dy), _d(x), _d(gamma), _d(dx0)
    fig = _Figures(f"ln_bwd D{D} rows{rows} skip{skip} det{int(det)}")

    def targets():
        return [_d(start[i].clone()) for i in range(3)]

    def sums(tag, t):
        for i, k in enumerate(("dgamma", "dbeta", "dx_colsum")):
            fig.close(f"{tag} {k}", t[i].double().cpu() - start[i].double(), sums_ref[k], LN_BWD_SUMS_TOL)

    if YARD:
        x32 = x.clone().requires_grad_(True)
        (Fn.layer_norm(x32, (D,), gamma, None, EPS) * dy).sum().backward()
        fig.yard("dx", dx0 + x32.grad, dx_ref)
        fig.yard("dgamma", (dy * xh.float()).sum(0), sums_ref["dgamma"])
        fig.yard("dx_colsum", (dx0 + x32.grad)[keep].sum(0), sums_ref["dx_colsum"])
    with _det(det):
        # fused kernel, in place (accumulate onto dx) and out of place (dx_in)
        buf, dx = _guarded(rows * D)
        dx.copy_(dx0_d.reshape(-1))
        t = targets()
        L.check(lib.mt_layernorm_bwd(L.ptr(dy_d), L.ptr(x_d), L.ptr(stats), L.ptr(gamma_d), L.ptr(dx), L.ptr(t[0]), L.ptr(t[1]), rows, D, 1,
                                     L.ptr(t[2]), skip, None, L.stream_ptr()), "mt_layernorm_bwd")
        torch.cuda.synchronize()
        fig.close("fused dx", dx.reshape(rows, D), dx_ref, LN_BWD_DX_TOL)
        sums("fused", t)
        buf2, dx2 = _guarded(rows * D)
        t2 = targets()
        L.check(lib.mt_layernorm_bwd(L.ptr(dy_d), L.ptr(x_d), L.ptr(stats), L.ptr(gamma_d), L.ptr(dx2), L.ptr(t2[0]), L.ptr(t2[1]), rows, D, 1,
                                     L.ptr(t2[2]), skip, L.ptr(dx0_d), L.stream_ptr()), "mt_layernorm_bwd (out of place)")
        torch.cuda.synchronize()
        fig.true("out of place: same dx, dx_in untouched", torch.equal(dx2, dx) and torch.equal(dx0_d.cpu(), dx0))
        fig.true("fused: nothing written outside dx", _bands_intact(buf) and _bands_intact(buf2))
        if det:
            fig.true("deterministic mode: fused sums bit-identical on a second run", all(torch.equal(a, b) for a, b in zip(t, t2)))
        # accumulate = 0: dx = LN'(dy) alone
        buf3, dx3 = _guarded(rows * D)
        t3 = targets()
        L.check(lib.mt_layernorm_bwd(L.ptr(dy_d), L.ptr(x_d), L.ptr(stats), L.ptr(gamma_d), L.ptr(dx3), L.ptr(t3[0]), L.ptr(t3[1]), rows, D, 0,
                                     None, 0, None, L.stream_ptr()), "mt_layernorm_bwd (no accumulate)")
        torch.cuda.synchronize()
        fig.close("fused dx, accumulate = 0", dx3.reshape(rows, D), xd.grad, LN_BWD_DX_TOL)
        # rows kernel (+ planes) and cols kernel
        buf4, dx4 = _guarded(rows * D)
        dxp = L.planes_empty(rows, D, dev)
        dxp.fill_(float("nan"))
        L.check(lib.mt_layernorm_bwd_rows(L.ptr(dy_d), L.ptr(x_d), L.ptr(stats), L.ptr(gamma_d), L.ptr(dx4), L.ptr(dx0_d), rows, D, L.ptr(dxp),
                                          L.stream_ptr()), "mt_layernorm_bwd_rows")
        t4 = targets()
        L.check(lib.mt_layernorm_bwd_cols(L.ptr(dy_d), L.ptr(x_d), L.ptr(stats), L.ptr(dx4), L.ptr(t4[0]), L.ptr(t4[1]), L.ptr(t4[2]), skip, rows,
                                          D, L.stream_ptr()), "mt_layernorm_bwd_cols")
        torch.cuda.synchronize()
        fig.close("rows dx", dx4.reshape(rows, D), dx_ref, LN_BWD_DX_TOL)
        fig.true("rows: dx_planes == split_planes_blk(dx), padding included", torch.equal(dxp, L.split_planes_blk(dx4.reshape(rows, D), rows, D)))
        fig.true("rows: nothing written outside dx", _bands_intact(buf4))
        sums("cols", t4)
        # rows + per-block partial sums, then the block-order reduce
        nb = lib.mt_layernorm_bwd_rows_blocks(rows)
        buf5, dx5 = _guarded(rows * D)
        pbuf, part = _guarded(nb * 3 * D)
        dxp5 = L.planes_empty(rows, D, dev)
        dxp5.fill_(float("nan"))
        rc = lib.mt_layernorm_bwd_rows_sums(L.ptr(dy_d), L.ptr(x_d), L.ptr(stats), L.ptr(gamma_d), L.ptr(dx5), L.ptr(dx0_d), rows, D, L.ptr(dxp5),
                                            L.ptr(part), skip, L.stream_ptr())
        torch.cuda.synchronize()
        if D > 512:
            fig.true("rows_sums refuses dim > 512 and writes nothing",
                     rc == MT_ERR_UNSUPPORTED and bool(torch.isnan(dx5).all()) and bool(torch.isnan(part).all()))
        else:
            L.check(rc, "mt_layernorm_bwd_rows_sums")
            res = []
            for _ in range(2):
                t5 = targets()
                L.check(lib.mt_layernorm_bwd_cols_reduce(L.ptr(part), nb, D, L.ptr(t5[0]), L.ptr(t5[1]), L.ptr(t5[2]), L.stream_ptr()), "cols_reduce")
                res.append(t5)
            torch.cuda.synchronize()
            fig.close("rows_sums dx", dx5.reshape(rows, D), dx_ref, LN_BWD_DX_TOL)
            fig.true("rows_sums: dx_planes == split_planes_blk(dx), padding included",
                     torch.equal(dxp5, L.split_planes_blk(dx5.reshape(rows, D), rows, D)))
            fig.true("rows_sums: nothing written outside dx / partials", _bands_intact(buf5) and _bands_intact(pbuf))
            sums("cols_reduce", res[0])
            fig.true("cols_reduce: run-to-run identical", all(torch.equal(a, b) for a, b in zip(res[0], res[1])))
            t6 = targets()
            L.check(lib.mt_layernorm_bwd_cols_reduce(L.ptr(part), nb, D, L.ptr(t6[0]), L.ptr(t6[1]), None, L.stream_ptr()), "cols_reduce")
            torch.cuda.synchronize()
            fig.true("cols_reduce: dx_colsum is optional", torch.equal(t6[0], res[0][0]) and torch.equal(t6[1], res[0][1])
                     and torch.equal(t6[2].cpu(), start[2]))
    fig.done()


# ---- 4. the classification head --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,det", [(1, False), (2, False), (5, False), (5, True)])
@pytest.mark.parametrize("classes", [1, 3])
@pytest.mark.parametrize("D", [64, 512, 1024])
def test_head_forward_and_backward_vs_fp64(D, classes, B, det):
    """mt_head_fwd / mt_head_bwd (the single-block kernel at B = 1 and in deterministic mode, one block per clip otherwise): only row 0
    of each clip is read and only row 0 of dx is written; the four parameter gradients accumulate onto non-zero starting values."""
    N = 3
    g = _gen(D + 10 * classes + B)
    x = torch.randn(B, N, D, generator=g) * 1.2 + 0.1
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.3
    w, bias = torch.randn(classes, D, generator=g) * D ** -0.5, torch.randn(classes, generator=g)
    dl = torch.randn(B, classes, generator=g)
    start = {"dgamma": torch.randn(D, generator=g), "dbeta": torch.randn(D, generator=g), "dw": torch.randn(classes, D, generator=g),
             "dbias": torch.randn(classes, generator=g)}

    def run(dt):
        p = {k: v.to(dt).requires_grad_(True) for k, v in (("x", x), ("gamma", gamma), ("beta", beta), ("w", w), ("bias", bias))}
        logits = Fn.linear(Fn.layer_norm(p["x"][:, 0], (D,), p["gamma"], p["beta"], EPS), p["w"], p["bias"])
        (logits * dl.to(dt)).sum().backward()
        return logits.detach(), p

    ref, p = run(torch.float64)
    x_d, gamma_d, beta_d, w_d, bias_d, dl_d = _d(x), _d(gamma), _d(beta), _d(w), _d(bias), _d(dl)
    fig = _Figures(f"head D{D} C{classes} B{B} det{int(det)}")
    lbuf, logits = _guarded(B * classes)
    L.check(L.get().mt_head_fwd(L.ptr(x_d), L.ptr(gamma_d), L.ptr(beta_d), L.ptr(w_d), L.ptr(bias_d), L.ptr(logits), B, N, D, classes, EPS,
                                L.stream_ptr()), "mt_head_fwd")
    torch.cuda.synchronize()
    fig.close("logits", logits.reshape(B, classes), ref, HEAD_FWD_TOL)
    fig.true("forward wrote only the logits", _bands_intact(lbuf))
    dbuf, dx = _guarded(B * N * D, CANARY)
    t = {k: _d(v.clone()) for k, v in start.items()}
    with _det(det):
        L.check(L.get().mt_head_bwd(L.ptr(dl_d), L.ptr(x_d), L.ptr(gamma_d), L.ptr(beta_d), L.ptr(w_d), L.ptr(dx), L.ptr(t["dgamma"]),
                                    L.ptr(t["dbeta"]), L.ptr(t["dw"]), L.ptr(t["dbias"]), B, N, D, classes, EPS, L.stream_ptr()), "mt_head_bwd")
        torch.cuda.synchronize()
    dx = dx.reshape(B, N, D)
    fig.close("dx row 0", dx[:, 0], p["x"].grad[:, 0], HEAD_BWD_TOL)
    fig.true("dx rows 1.. keep the canary", bool((dx[:, 1:] == CANARY).all()) and _bands_intact(dbuf))
    refs = {"dgamma": p["gamma"].grad, "dbeta": p["beta"].grad, "dw": p["w"].grad, "dbias": p["bias"].grad}
    for k in refs:
        fig.close(k, t[k].double().cpu() - start[k].double(), refs[k], HEAD_BWD_TOL)
    if YARD:
        r32, p32 = run(torch.float32)
        fig.yard("logits", r32, ref)
        fig.yard("dx row 0", p32["x"].grad[:, 0], p["x"].grad[:, 0])
        for k, pk in (("dgamma", "gamma"), ("dbeta", "beta"), ("dw", "w"), ("dbias", "bias")):       # accumulated in fp32 like the kernel's
            fig.yard(k, (start[k] + p32[pk].grad).double() - start[k].double(), refs[k])
    fig.done()


@pytest.mark.parametrize("D,classes", [(96, 1), (64, 65), (1088, 1)])
def test_head_backward_refusals_write_nothing(D, classes):
    B, N = 2, 3
    x = torch.randn(B, N, D, device=dev)
    v, wt = torch.ones(D, device=dev), torch.ones(classes, D, device=dev)
    dl = torch.ones(B, classes, device=dev)
    dbuf, dx = _guarded(B * N * D, CANARY)
    t = [torch.full((D,), CANARY, device=dev), torch.full((D,), CANARY, device=dev), torch.full((classes, D), CANARY, device=dev),
         torch.full((classes,), CANARY, device=dev)]
    rc = L.get().mt_head_bwd(L.ptr(dl), L.ptr(x), L.ptr(v), L.ptr(v), L.ptr(wt), L.ptr(dx), L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]),
                             B, N, D, classes, EPS, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == MT_ERR_ARG
    assert bool((dx == CANARY).all()) and _bands_intact(dbuf) and all(bool((a == CANARY).all()) for a in t)


# ---- 5. the embeddings -------------------------------------------------------------------------------------------------------------------

SIZE_ROWS = 21


def _embed_case(B, F, D, with_positions, seed):
    g = _gen(seed)
    N = 1 + F * n
    x0 = torch.randn(B, N, D, generator=g)
    cls = torch.randn(D, generator=g)
    if with_positions:       # the frame number per token: every position row is shared by 49 tokens (and by the clips)
        pos_rows = F + 3
        frames = torch.arange(1, F + 1).repeat_interleave(n)
        positions = torch.stack([torch.cat((torch.zeros(1, dtype=torch.int64), (frames + b) % pos_rows)) for b in range(B)])
    else:                    # positions = NULL: the token index; the table has exactly N rows, so N - 1 is its last row
        pos_rows, positions = N, None
    pos_emb, size_emb = torch.randn(pos_rows, D, generator=g), torch.randn(SIZE_ROWS, D, generator=g)
    sizes = torch.randint(0, SIZE_ROWS, (B, F), generator=g, dtype=torch.int32)
    sizes[0, 0], sizes[0, 1], sizes[-1, -1], sizes[-1, -2] = 20, 0, 0, 20        # both ends of the table, and slots with bucket 0
    pidx = positions if positions is not None else torch.arange(N).expand(B, N)
    sidx = torch.cat((torch.zeros(B, 1, dtype=torch.int64), sizes.long().repeat_interleave(n, dim=1)), dim=1)
    return x0, cls, pos_emb, size_emb, positions, sizes, pidx, sidx, pos_rows


def _embed_fwd(x0, cls_d, pos_d, size_d, positions_d, sizes_d, B, F, D, pos_rows, size_rows):
    N = 1 + F * n
    xbuf, x = _guarded(B * N * D)
    x.copy_(_d(x0).reshape(-1))
    x.reshape(B, N, D)[:, 0] = float("nan")               # the cls rows of the input are not read
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.get().mt_embed_fwd(L.ptr(x), L.ptr(cls_d), L.ptr(pos_d), L.ptr(size_d), L.ptr(positions_d), L.ptr(sizes_d), B, F, n, D, pos_rows,
                                 size_rows, L.ptr(err), L.stream_ptr()), "mt_embed_fwd")
    torch.cuda.synchronize()
    assert _bands_intact(xbuf), "mt_embed_fwd wrote outside x"
    return x.reshape(B, N, D), int(err.item())


@pytest.mark.parametrize("with_positions", [True, False])
@pytest.mark.parametrize("D", [64, 320, 512])
@pytest.mark.parametrize("B,F", [(1, 8), (3, 16)])
def test_embed_forward_vs_fp64(B, F, D, with_positions):
    """x[b, 0] = cls + pos_emb[.] + size_emb[0], x[b, 1 + t] += pos_emb[.] + size_emb[bucket of the token's frame], against fp64; the
    error flag stays 0 for in-range indices -- also when the size table is absent (enable-size-emb False) and `sizes` is still passed:
    the buckets are then not looked at."""
    x0, cls, pos_emb, size_emb, positions, sizes, pidx, sidx, pos_rows = _embed_case(B, F, D, with_positions, 7 * B + F + D)
    base = x0.double().clone()
    base[:, 0] = cls.double()
    base = base + pos_emb.double()[pidx]
    ref = base + size_emb.double()[sidx]
    cls_d, pos_d, size_d, sizes_d = _d(cls), _d(pos_emb), _d(size_emb), _d(sizes)
    positions_d = _d(positions) if positions is not None else None
    fig = _Figures(f"embed_fwd B{B} F{F} D{D} pos{int(with_positions)}")
    x, err = _embed_fwd(x0, cls_d, pos_d, size_d, positions_d, sizes_d, B, F, D, pos_rows, SIZE_ROWS)
    _out_sections(fig, "x", x, ref, EMBED_FWD_TOL)
    fig.true("in-range indices: error flag 0", err == 0)
    if YARD:
        b32 = x0.clone()
        b32[:, 0] = cls
        fig.yard("x", b32 + pos_emb[pidx] + size_emb[sidx], ref)
    # no size table, buckets still given
    x, err = _embed_fwd(x0, cls_d, pos_d, None, positions_d, sizes_d, B, F, D, pos_rows, 0)
    _out_sections(fig, "x (size_emb = NULL, sizes given)", x, base, EMBED_FWD_TOL)
    fig.true("size_emb = NULL, sizes given: error flag 0", err == 0)
    # neither
    x, err = _embed_fwd(x0, cls_d, pos_d, None, positions_d, None, B, F, D, pos_rows, 0)
    _out_sections(fig, "x (size_emb = NULL, sizes = NULL)", x, base, EMBED_FWD_TOL)
    fig.true("size_emb = NULL, sizes = NULL: error flag 0", err == 0)
    # a real out-of-range bucket is still flagged (bit 1) and clamped into the table
    bad = sizes.clone()
    bad[0, 2] = SIZE_ROWS
    x, err = _embed_fwd(x0, cls_d, pos_d, size_d, positions_d, _d(bad), B, F, D, pos_rows, SIZE_ROWS)
    sidx_c = torch.cat((torch.zeros(B, 1, dtype=torch.int64), bad.long().clamp(max=SIZE_ROWS - 1).repeat_interleave(n, dim=1)), dim=1)
    _out_sections(fig, "x (clamped bucket)", x, base + size_emb.double()[sidx_c], EMBED_FWD_TOL)
    fig.true("out-of-range bucket: bit 1 of the error flag", err == 2)
    fig.done()


@pytest.mark.parametrize("with_positions", [True, False])
@pytest.mark.parametrize("D", [64, 320, 512])
@pytest.mark.parametrize("B,F", [(1, 8), (3, 16)])
def test_embed_backward_vs_fp64(B, F, D, with_positions):
    """mt_embed_bwd against index_add_ in fp64, added onto non-zero tables: the slots kernel (320 columns: its 256-column stride leaves
    a tail) and deterministic mode's limb scatter + decode, which is bit-identical on a second run."""
    N = 1 + F * n
    _, _, pos_emb, size_emb, positions, sizes, pidx, sidx, pos_rows = _embed_case(B, F, D, with_positions, 7 * B + F + D)
    g = _gen(3 * B + F + D)
    dx = torch.randn(B, N, D, generator=g)
    start = {"dcls": torch.randn(D, generator=g), "dpos": torch.randn(pos_rows, D, generator=g), "dsize": torch.randn(SIZE_ROWS, D, generator=g)}

    def ref_in(dt):
        flat = dx.to(dt).reshape(B * N, D)
        return {"dcls": dx.to(dt)[:, 0].sum(0), "dpos": torch.zeros(pos_rows, D, dtype=dt).index_add_(0, pidx.reshape(-1), flat),
                "dsize": torch.zeros(SIZE_ROWS, D, dtype=dt).index_add_(0, sidx.reshape(-1), flat)}

    ref = ref_in(torch.float64)
    dx_d, sizes_d = _d(dx), _d(sizes)
    positions_d = _d(positions) if positions is not None else None
    fig = _Figures(f"embed_bwd B{B} F{F} D{D} pos{int(with_positions)}")
    if YARD:
        r32 = ref_in(torch.float32)
        for k in ref:
            fig.yard(k, r32[k], ref[k])

    def run(with_size=True):
        bufs = {k: _guarded(v.numel()) for k, v in start.items()}
        for k, v in start.items():
            bufs[k][1].copy_(_d(v).reshape(-1))
        L.check(L.get().mt_embed_bwd(L.ptr(dx_d), L.ptr(bufs["dcls"][1]), L.ptr(bufs["dpos"][1]), L.ptr(bufs["dsize"][1]) if with_size else None,
                                     L.ptr(positions_d), L.ptr(sizes_d), B, F, n, D, pos_rows, SIZE_ROWS if with_size else 0, L.stream_ptr()),
                "mt_embed_bwd")
        torch.cuda.synchronize()
        assert all(_bands_intact(b) for b, _ in bufs.values()), "mt_embed_bwd wrote outside its tables"
        return {k: bufs[k][1].reshape(start[k].shape).clone() for k in start}

    for det in (False, True):
        tag = "deterministic" if det else "default"
        with _det(det):
            got = run()
            for k in ref:
                fig.close(f"{tag} {k}", got[k].double().cpu() - start[k].double(), ref[k], EMBED_BWD_TOL)
            if det:
                again = run()
                fig.true("deterministic mode: second run bit-identical", all(torch.equal(got[k], again[k]) for k in got))
            nos = run(with_size=False)            # no size table (buckets still given): the other two gradients unchanged in value
            for k in ("dcls", "dpos"):
                fig.close(f"{tag} {k} (dsize_emb = NULL)", nos[k].double().cpu() - start[k].double(), ref[k], EMBED_BWD_TOL)
            fig.true(f"{tag}: dsize_emb = NULL leaves the size table alone", torch.equal(nos["dsize"].cpu(), start["dsize"]))
    fig.done()


# ---- 6. column sums -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("N_", [1, 70, 512])
@pytest.mark.parametrize("M", [1, 257, 1000])
def test_colsum_vs_fp64(M, N_, mapped):
    """out[c] += sum_m A[map(m) * lda + c] with lda > N, onto a non-zero out; the row map (392, 393, 1) is the one that skips the cls
    row of every clip.  Default (atomics) and deterministic mode (bit-identical on a second run); N = 1 and 70 leave the last 64-column
    group of deterministic mode's log partly outside out, which its reduce must not touch -- not even by adding 0 (the guard bands)."""
    lda = N_ + 5
    gin, gout, off = (392, 393, 1) if mapped else (0, 0, 0)
    src_rows = ((M - 1) // 392) * 393 + 1 + (M - 1) % 392 + 1 if mapped else M
    g = _gen(M + N_)
    A = torch.randn(src_rows + 1, lda, generator=g)
    start = torch.randn(N_, generator=g)
    rows = torch.arange(M)
    if mapped:
        rows = (rows // gin) * gout + off + rows % gin
    ref = A.double()[rows, :N_].sum(0)
    A_d = _d(A)
    fig = _Figures(f"colsum M{M} N{N_} map{int(mapped)}")
    if YARD:
        fig.yard("out", A[rows, :N_].sum(0), ref)
    for det in (False, True):
        res = []
        with _det(det):
            for _ in range(2):
                buf, out = _guarded(N_)
                out.copy_(_d(start))
                L.check(L.get().mt_colsum(L.ptr(A_d), lda, L.RowMap(gin, gout, off), M, N_, L.ptr(out), L.stream_ptr()), "mt_colsum")
                torch.cuda.synchronize()
                fig.true("nothing written outside out", _bands_intact(buf))
                res.append(out.clone())
        fig.close(f"{'deterministic' if det else 'default'} out", res[0].double().cpu() - start.double(), ref, COLSUM_TOL)
        if det:
            fig.true("deterministic mode: second run bit-identical", torch.equal(res[0], res[1]))
    fig.done()


# ---- 7. attention aggregation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale_factor", [1, 50000])
@pytest.mark.parametrize("BH", [1, 8, 24])
@pytest.mark.parametrize("F", [8, 16, 32])
def test_attention_aggregate_vs_fp64(F, BH, scale_factor):
    """mt_attn_aggregate on genuine probability rows: per token the maximum over (batch * heads), numpy.array_split into F chunks
    (N = 1 + 49 F is never a multiple of F: the first chunk is one longer), mean * scale_factor, softmax; rows space / time / sum."""
    N = 1 + F * n
    g = _gen(F + BH)
    space = (torch.randn(BH, N, generator=g) * 2).softmax(-1)
    time_ = (torch.randn(BH, N, generator=g) * 2).softmax(-1)

    def ref_in(dt):
        ms, mt = space.to(dt).numpy().max(0), time_.to(dt).numpy().max(0)
        rows = []
        for row in (ms, mt, ms + mt):
            v = np.array([c.mean() * dt_scale(dt) for c in np.array_split(row, F)])
            e = np.exp(v - v.max())
            rows.append(e / e.sum())
        return torch.from_numpy(np.stack(rows))

    def dt_scale(dt):
        return np.float64(scale_factor) if dt == torch.float64 else np.float32(scale_factor)

    ref = ref_in(torch.float64)
    space_d, time_d = _d(space), _d(time_)
    buf, out = _guarded(3 * F)
    L.check(L.get().mt_attn_aggregate(L.ptr(space_d), L.ptr(time_d), L.ptr(out), BH, N, F, float(scale_factor), L.stream_ptr()),
            "mt_attn_aggregate")
    torch.cuda.synchronize()
    fig = _Figures(f"aggregate s{scale_factor} F{F} BH{BH}")
    out = out.reshape(3, F)
    for i, name in enumerate(("space", "time", "combined")):
        fig.close(name, out[i], ref[i], AGG_TOL[scale_factor])
    if YARD:
        fig.yard("all rows", ref_in(torch.float32), ref)
    fig.true("nothing written outside out", _bands_intact(buf))
    fig.done()
