"""The Size-Invariant TimeSformer at num-patches other than 49 (1 <= n <= 100).

Part 1 calls mt_attn_fwd / mt_attn_bwd through the C ABI, the way tests/test_gpu_tsf_ops.py does at n = 49 (guard bands round every
output, NaN pre-fill, every figure printed before anything is asserted), at the sizes where the space-attention kernels change tile
or kernel: n <= 63 runs the 2 x 2-tile MFMA kernels, 64 <= n <= 95 the query-walking kernels with three key tiles, 96 <= n <= 100 with
four.  The reference is tests/tsf_ref.py in fp64.  The gate on a compared section is max(2 x yardstick, floor): the yardstick is the
error of the SAME reference evaluated in fp32 on the CPU for the same inputs on that section (the n = 49 kernels measured 0.4 .. 0.9 of
it, and an MFMA's summation order is not the CPU's, hence the factor 2); the floor is the n = 49 gate of that regime, because the
yardstick of a small section can come out near zero by luck.

Part 2 runs the model (forward, backward, plans, attention aggregation, the extractor at 256 x 256) against oracle/mintime_oracle.py
and the two fixtures recorded from the reference at 16 and 64 patches, under tests/util.py::REL_TOL like tests/test_gpu_tsf.py."""
from contextlib import contextmanager
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as Fn

from mintime_amd import SizeInvariantTimeSformer, arch, harness, synth
from mintime_amd import lib as L
from oracle import mintime_oracle as O

from . import tsf_ref as R
from .util import REL_TOL, golden, rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)

GUARD_BITS = -2 ** 31          # the guard bands hold -0.0: any store shows, and so does a read-modify-write that adds +0.0
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3          # csrc/common.hpp
DH = 64
SCALE = DH ** -0.5

# the floors: ATTN_FWD_TOL / ATTN_BWD_TOL of tests/test_gpu_tsf_ops.py (the n = 49 gates), as they stand there
ATTN_FWD_TOL = {"moderate": 9e-7, "peaky": 5e-6, "negative": 2e-5}
ATTN_BWD_TOL = {"moderate": 9e-7, "peaky": 7e-6, "negative": 9e-5}


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


def _guarded(numel, fill=float("nan")):
    """A device buffer of `numel` floats holding `fill`, between two 64-element guard bands (an over-run shows in the bands)."""
    buf = torch.full((numel + 128,), -0.0, dtype=torch.float32, device=dev)
    body = buf[64:64 + numel]
    body.fill_(fill)
    return buf, body


def _bands_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[:64] == GUARD_BITS).all() and (bits[-64:] == GUARD_BITS).all())


class _Figures:
    """Collects the figures of one test, prints each before anything is asserted, then fails on all that missed."""

    def __init__(self, what, floor):
        self.what, self.floor, self.bad = what, floor, []

    def close(self, name, got, ref, ref32):
        """kernel error, yardstick (the fp32 CPU evaluation's error) and gate = max(2 x yardstick, floor) of one section."""
        e, y = rel_err(got, ref), rel_err(ref32, ref)
        gate = max(2.0 * y, self.floor)
        print(f"FIG {self.what} | {name} | {e:.3e} | yardstick {y:.3e} | gate {gate:.3e} | ratio {e / max(y, 1e-30):.2f}")
        if not e <= gate:
            self.bad.append(f"{name}: {e:.3e} > {gate:.3e}")

    def true(self, name, cond):
        if not bool(cond):
            print(f"FIG {self.what} | {name} | FALSE")
            self.bad.append(name)

    def done(self):
        assert not self.bad, f"{self.what}: " + "; ".join(self.bad)


# ---- 1. the divided-attention core at n != 49 ------------------------------------------------------------------------------------

# (n, B, H, F)
ATTN_CASES = [(1, 2, 8, 8),       # two keys per group; the factored cls hand-over does not fit (16 scratch rows needed, 8 present)
              (2, 2, 8, 8),       # ... fits exactly (16 rows of 16)
              (4, 2, 2, 8),       # far below one tile
              (31, 2, 2, 8),      # 32 keys fill one key tile exactly
              (32, 2, 2, 8),      # the first key of key tile 2
              (33, 2, 2, 8),      # the first query of query tile 2
              (63, 2, 2, 8),      # 64 keys: the last size the 2 x 2 kernels hold
              (64, 2, 2, 8),      # the query-walking kernels: a third key tile holding one key
              (65, 2, 2, 8),      # a third query tile holding one query
              (81, 2, 2, 8),      # 9 x 9
              (96, 2, 2, 8),      # three full query tiles; a fourth key tile holding one key
              (100, 2, 2, 8),     # the upper end
              (100, 1, 1, 16),    # ... with the time path's second instantiation
              (100, 3, 8, 8)]     # ... with the model's head count
ATTN_MASKS = ["ones", "ragged", "zeroclip"]
_BLOCKS = {8: [3, 3, 2], 16: [7, 5, 4]}


def _regimes(n, B, H, F):
    return ["moderate", "peaky"] + (["negative"] if (n in (64, 100) and (B, H, F) == (2, 2, 8)) else [])


ATTN_PARAMS = [(n, B, H, F, r) for (n, B, H, F) in ATTN_CASES for r in _regimes(n, B, H, F)]


def _attn_masks(kind, B, F, g):
    """(mask [B, F] bool, ident [B, F, F] bool, index of the clip whose mask is all zero or None)."""
    mask = torch.ones(B, F, dtype=torch.bool)
    ident = torch.ones(B, F, F, dtype=torch.bool)
    zero_clip = None
    if kind == "ragged":             # random (asymmetric) identities, the last frames padding, one more padded frame in the middle
        ident = torch.rand(B, F, F, generator=g) < 0.5
        mask[:, F - max(1, _BLOCKS[F][-1] // 2):] = False
        mask[:, 1] = False
    elif kind == "zeroclip":
        o = 0
        ident = torch.zeros(B, F, F, dtype=torch.bool)
        for k in _BLOCKS[F]:
            ident[:, o:o + k, o:o + k] = True
            o += k
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


def _attn_case(n, B, H, F, kind, regime):
    g = _gen(100000 * n + 1000 * B + 100 * H + F)
    N = 1 + F * n
    mask, ident, zero_clip = _attn_masks(kind, B, F, g)
    qkv = _attn_qkv(regime, B, N, H, g)
    dout = torch.randn(B, N, H * DH, generator=g)
    return qkv, dout, mask, ident, zero_clip


def _attn_fwd(qkv_d, mask_d, ident_d, n, B, H, F, mode, fp32=True, att=True, planes=False, check=True):
    N, inner = 1 + F * n, H * DH
    obuf, o = _guarded(B * N * inner) if fp32 else (None, None)
    abuf, a = _guarded(B * H * N) if att else (None, None)
    op = None
    if planes:
        op = L.planes_empty(B * N, inner, dev)
        op.fill_(float("nan"))
    rc = L.get().mt_attn_fwd(L.ptr(qkv_d), L.ptr(o), L.ptr(a), L.ptr(mask_d), L.ptr(ident_d), B, H, F, n, mode, SCALE, L.ptr(op),
                             L.stream_ptr())
    torch.cuda.synchronize()
    assert (obuf is None or _bands_intact(obuf)) and (abuf is None or _bands_intact(abuf)), "mt_attn_fwd wrote outside its outputs"
    if not check:
        return rc, o, a, op
    L.check(rc, "mt_attn_fwd")
    return (o.reshape(B, N, inner) if fp32 else None), (a.reshape(B * H, N) if att else None), op


def _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode, planes=False, check=True):
    N, inner = 1 + F * n, H * DH
    buf, dqkv = _guarded(B * N * 3 * inner)
    dp = None
    if planes:
        dp = L.planes_empty(B * N, 3 * inner, dev)
        dp.fill_(float("nan"))
    rc = L.get().mt_attn_bwd(L.ptr(qkv_d), L.ptr(dout_d), L.ptr(dqkv), L.ptr(mask_d), L.ptr(ident_d), B, H, F, n, mode, SCALE,
                             L.ptr(dp), L.stream_ptr())
    torch.cuda.synchronize()
    assert _bands_intact(buf), "mt_attn_bwd wrote outside dqkv"
    if not check:
        return rc, dqkv, dp
    L.check(rc, "mt_attn_bwd")
    return dqkv.reshape(B, N, 3 * inner), dp


def _planes_padding_is_zero(planes, rows, cols):
    full = L.planes_to_float(planes, planes.shape[1] * 32, cols)
    return not bool(torch.isnan(planes.float()).any()) and float(full[rows:].abs().sum()) == 0.0


def _out_sections(fig, tag, got, ref, ref32, mode):
    fig.close(f"{tag} cls rows", got[:, 0], ref[:, 0], ref32[:, 0])
    if mode != 2:                                    # mode 2 writes row 0 of every clip only
        fig.close(f"{tag} patch rows", got[:, 1:], ref[:, 1:], ref32[:, 1:])


def _grad_sections(fig, tag, got, ref, ref32, mode):
    for name, gt, rf, r32 in zip(("dq", "dk", "dv"), got.chunk(3, dim=-1), ref.chunk(3, dim=-1), ref32.chunk(3, dim=-1)):
        for rows, sl in (("cls rows", slice(0, 1)), ("patch rows", slice(1, None))):
            if mode == 2 and name == "dq" and rows == "patch rows":
                continue                             # mode 2 does not write the dq section of the patch rows
            fig.close(f"{tag} {name} {rows}", gt[:, sl], rf[:, sl], r32[:, sl])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ATTN_MASKS)
@pytest.mark.parametrize("n,B,H,F,regime", ATTN_PARAMS)
def test_attention_forward_vs_fp64(n, B, H, F, regime, kind, mode):
    """out (cls rows, patch rows) and cls_att of mt_attn_fwd against tests/tsf_ref.py in fp64; masked keys get exactly zero attention,
    a clip whose mask is all zero an exactly one-hot cls_att; the plane output is the exact split of the fp32 output."""
    N, inner = 1 + F * n, H * DH
    qkv, _, mask, ident, zero_clip = _attn_case(n, B, H, F, kind, regime)
    ref, ref_att = R.attn_ref(qkv.double(), mask, ident, H, F, n, mode, SCALE)
    r32, a32 = R.attn_ref(qkv, mask, ident, H, F, n, mode, SCALE)
    qkv_d, mask_d, ident_d = _d(qkv), _d(mask.to(torch.uint8)), _d(ident.to(torch.uint8))
    out, att, _ = _attn_fwd(qkv_d, mask_d, ident_d, n, B, H, F, mode)
    fig = _Figures(f"attn_fwd n{n} {regime} B{B} H{H} F{F} {kind} mode{mode}", ATTN_FWD_TOL[regime])
    _out_sections(fig, "out", out, ref, r32, mode)
    fig.close("cls_att", att, ref_att, a32)
    att_c = att.cpu()
    keep = torch.cat((torch.ones(B, 1, dtype=torch.bool), mask.repeat_interleave(n, dim=1)), dim=1).repeat_interleave(H, dim=0)
    fig.true("masked keys are exactly 0 in cls_att", (att_c[~keep] == 0).all())
    rowsum = float((att_c.double().sum(1) - 1.0).abs().max())
    sum_gate = max(2.0 * float((a32.double().sum(1) - 1.0).abs().max()), ATTN_FWD_TOL[regime])
    print(f"FIG {fig.what} | cls_att row sums - 1 | {rowsum:.3e} | gate {sum_gate:.3e}")
    fig.true("cls_att rows sum to 1", rowsum <= sum_gate)
    if zero_clip is not None:
        z = att_c[zero_clip * H:(zero_clip + 1) * H]
        fig.true("all-zero mask: cls_att is exactly one-hot", bool((z[:, 0] == 1).all() and (z[:, 1:] == 0).all()))
    if mode == 2:
        fig.true("mode 2: the patch rows are not written", torch.isnan(out[:, 1:]).all())
    else:   # plane output: alone (out = NULL) and together with the fp32 output
        _, _, op = _attn_fwd(qkv_d, mask_d, ident_d, n, B, H, F, mode, fp32=False, att=False, planes=True)
        pf = L.planes_to_float(op, B * N, inner)
        fig.true("planes == split of the fp32 output", torch.equal(pf, out.reshape(B * N, inner)))
        fig.true("plane padding rows are zero", _planes_padding_is_zero(op, B * N, inner))
        _out_sections(fig, "planes", pf.reshape(B, N, inner), ref, r32, mode)
        out2, _, op2 = _attn_fwd(qkv_d, mask_d, ident_d, n, B, H, F, mode, att=False, planes=True)
        fig.true("fp32 + planes in one call: same bits", torch.equal(out2, out) and torch.equal(op2, op))
    fig.done()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ATTN_MASKS)
@pytest.mark.parametrize("n,B,H,F,regime", ATTN_PARAMS)
def test_attention_backward_vs_fp64(n, B, H, F, regime, kind, mode):
    """dq, dk, dv of mt_attn_bwd on cls rows and on patch rows against autograd of tests/tsf_ref.py in fp64: default mode,
    deterministic mode (twice: bit-identical) and the plane output, whose cls hand-over is factored only where its scratch rows fit
    into the clip (n = 1 at 8 heads: they do not, and an over-run would show in the next clip's rows and in the guard band)."""
    N, inner = 1 + F * n, H * DH
    qkv, dout, mask, ident, zero_clip = _attn_case(n, B, H, F, kind, regime)
    ref = R.attn_bwd_ref(qkv.double(), dout.double(), mask, ident, H, F, n, mode, SCALE)
    r32 = R.attn_bwd_ref(qkv, dout, mask, ident, H, F, n, mode, SCALE)
    qkv_d, dout_d, mask_d, ident_d = _d(qkv), _d(dout), _d(mask.to(torch.uint8)), _d(ident.to(torch.uint8))
    fig = _Figures(f"attn_bwd n{n} {regime} B{B} H{H} F{F} {kind} mode{mode}", ATTN_BWD_TOL[regime])
    planes = mode != 2                                # (plane output is refused in mode 2)
    with _det(False):
        got, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode)
        _grad_sections(fig, "default", got, ref, r32, mode)
        if planes:
            _, dp = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode, planes=True)
            gp = L.planes_to_float(dp, B * N, 3 * inner).reshape(B, N, 3 * inner)
            _grad_sections(fig, "planes", gp, ref, r32, mode)
            fig.true("plane padding rows are zero", _planes_padding_is_zero(dp, B * N, 3 * inner))
            fig.true("planes: patch rows have one owner, same values as fp32", torch.equal(gp[:, 1:], got[:, 1:]))
    with _det(True):
        d1, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode)
        d2, _ = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode)
        _grad_sections(fig, "deterministic", d1, ref, r32, mode)
        same = torch.equal(d1[:, :1], d2[:, :1]) and torch.equal(d1[:, 1:, inner:], d2[:, 1:, inner:]) if mode == 2 else torch.equal(d1, d2)
        fig.true("deterministic mode: second run bit-identical", same)
        if planes:
            _, p1 = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode, planes=True)
            _, p2 = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode, planes=True)
            _grad_sections(fig, "deterministic planes", L.planes_to_float(p1, B * N, 3 * inner).reshape(B, N, 3 * inner), ref, r32, mode)
            fig.true("deterministic mode: plane output bit-identical", torch.equal(p1, p2))
    if mode == 2:
        fig.true("mode 2: the dq section of the patch rows is not written", torch.isnan(got[:, 1:, :inner]).all())
    if zero_clip is not None and mode == 0:
        for tag, t in (("default", got), ("planes", gp), ("deterministic", d1)):
            fig.true(f"all-zero mask, time mode ({tag}): dk / dv of the clip's patch keys are exactly 0",
                     (t[zero_clip, 1:, inner:] == 0).all())
    fig.done()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("n", [0, 101])
def test_attention_refuses_num_patches_outside_1_to_100(n, planes, mode):
    """n = 0 and n = 101 are refused by both entry points with an error code, before anything is launched: every output still holds
    its NaN fill and the guard bands are intact."""
    B, H, F = 2, 2, 8
    N, inner = 1 + F * n, H * DH
    g = _gen(n)
    qkv_d, dout_d = _d(torch.randn(B, N, 3 * inner, generator=g)), _d(torch.randn(B, N, inner, generator=g))
    mask_d, ident_d = _d(torch.ones(B, F, dtype=torch.uint8)), _d(torch.ones(B, F, F, dtype=torch.uint8))
    rc, o, a, op = _attn_fwd(qkv_d, mask_d, ident_d, n, B, H, F, mode, planes=planes, check=False)
    assert rc in (MT_ERR_UNSUPPORTED, MT_ERR_ARG), rc
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(a).all()) and (op is None or bool(torch.isnan(op.float()).all()))
    rc, dqkv, dp = _attn_bwd(qkv_d, dout_d, mask_d, ident_d, n, B, H, F, mode, planes=planes, check=False)
    assert rc in (MT_ERR_UNSUPPORTED, MT_ERR_ARG), rc
    assert bool(torch.isnan(dqkv).all()) and (dp is None or bool(torch.isnan(dp.float()).all()))


# ---- 2. the model at num-patches 1 .. 100 ---------------------------------------------------------------------------------------

HEADS = 8
TSF_HIGH_GRAD_TOL = min(2 * 5.385e-4, REL_TOL)      # tier high's own gate: tests/test_gpu_precision.py, as it stands there


def _close(got, ref, tol, what):
    e = rel_err(got, ref)
    print(f"FIG model | {what} | {e:.3e} | tol {tol:.0e}")
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def _cfg(C, Fr, hw):
    return arch.default_tsf_config(C, Fr, num_patches=hw * hw, image_size=32 * hw)


def _build(cfg, seed, require_attention=False):
    model = SizeInvariantTimeSformer(config=cfg, require_attention=require_attention)
    sd = synth.tsf_state(cfg, seed)
    model.load_state_dict(sd, strict=True)
    return model.cuda(), sd


def _kw(aux):
    return dict(mask=aux["mask"].cuda(), identities_mask=aux["identities_mask"].cuda(), size_embedding=aux["size_embedding"],
                positions=aux["positions"].cuda())


def _fixture_inputs(g):
    B, Fr, C, hw = int(g["batch"]), int(g["frames"]), int(g["channels"]), int(g["hw"])
    feats = synth.features(B, Fr, C, int(g["seed"]), hw=hw)
    aux = synth.clip_inputs(B, Fr, int(g["identities"]), int(g["seed"]), ragged=bool(g["ragged"]), with_video=False, num_patches=hw * hw)
    return B, Fr, C, hw, feats, aux


@pytest.mark.parametrize("name", ["tsf_p16", "tsf_p64"])
def test_forward_matches_reference_fixture(name):
    g = golden(name)
    B, Fr, C, hw, feats, aux = _fixture_inputs(g)
    model, _ = _build(_cfg(C, Fr, hw), int(g["seed"]), require_attention=True)
    with torch.no_grad():
        logits, (s_att, t_att) = model(feats.cuda(), **_kw(aux))
    assert logits.shape == (B, 1) and s_att.shape == (B * HEADS, 1, 1 + Fr * hw * hw) and t_att.shape == s_att.shape
    _close(logits, g["logits"], REL_TOL, f"{name} logits vs reference")
    _close(s_att, g["space_att"], REL_TOL, f"{name} space cls attention vs reference")
    _close(t_att, g["time_att"], REL_TOL, f"{name} time cls attention vs reference")
    ref = torch.as_tensor(g["logits"])
    assert bool(((logits.cpu() - ref).abs() <= 1e-3 * ref.abs() + 1e-5).all())          # the elementwise gate of SURVEY §8c
    # masked keys get exactly zero cls attention
    keep = torch.cat([torch.ones(B, 1, dtype=torch.bool), aux["mask"].repeat_interleave(hw * hw, 1)], 1)
    keep = keep[:, None].expand(-1, HEADS, -1).reshape(-1, 1, keep.shape[-1])
    assert float(s_att.cpu()[~keep].abs().max()) == 0.0 and float(t_att.cpu()[~keep].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["tsf_p16", "tsf_p64"])
def test_backward_matches_reference_fixture(name):
    g = golden(name)
    B, Fr, C, hw, feats, aux = _fixture_inputs(g)
    model, _ = _build(_cfg(C, Fr, hw), int(g["seed"]))
    x = feats.cuda().requires_grad_(True)
    out = model(x, **_kw(aux))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out.cpu(), aux["labels"].reshape(-1, 1))
    loss.backward()
    _close(loss, g["loss"], REL_TOL, f"{name} loss")
    named = dict(model.named_parameters())
    for k in g.files:
        if k.startswith("gnorm."):
            key = k[len("gnorm."):]
            assert named[key].grad is not None, key
            _close(named[key].grad.norm(), g[k], REL_TOL, f"{name} {k}")
            if "gslice." + key in g.files:
                _close(named[key].grad.reshape(-1)[:256], g["gslice." + key], REL_TOL, f"{name} gslice.{key}")
    _close(named["pos_emb.weight"].grad[:8], g["gslice.pos_emb.rows"], REL_TOL, f"{name} pos_emb grad rows")
    _close(named["size_emb.weight"].grad[:21], g["gslice.size_emb.rows"], REL_TOL, f"{name} size_emb grad rows")
    assert float(named["pos_emb.weight"].grad[Fr * hw * hw + 1:].abs().max()) == 0.0
    _close(x.grad.norm(), g["dfeats_norm"], REL_TOL, f"{name} dfeats norm")
    _close(x.grad.permute(0, 1, 3, 4, 2).reshape(-1)[:512], g["dfeats_slice"], REL_TOL, f"{name} dfeats slice")


SEED = 5


def _weights(B):
    return torch.linspace(1.0, -0.7, B).reshape(B, 1) if B > 1 else torch.ones(1, 1)


@lru_cache(maxsize=None)
def _oracle(B, Fr, C, hw, ids):
    """(parameter gradients by name, dfeatures, logits) of sum(logits * w) by autograd over the CPU oracle; shared, never modified."""
    cfg = _cfg(C, Fr, hw)
    sd = synth.tsf_state(cfg, SEED)
    feats = synth.features(B, Fr, C, SEED, hw=hw)
    aux = synth.clip_inputs(B, Fr, ids, SEED, ragged=True, with_video=False, num_patches=hw * hw)
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = feats.clone().requires_grad_(True)
    oout = O.tsf_forward(osd, cfg, xo, aux["mask"], aux["identities_mask"], aux["size_embedding"], aux["positions"])
    (oout * _weights(B)).sum().backward()
    return {k: v.grad.detach() for k, v in osd.items()}, xo.grad.detach(), oout.detach()


def _model_and_inputs(B, Fr, C, hw, ids):
    model, _ = _build(_cfg(C, Fr, hw), SEED)
    feats = synth.features(B, Fr, C, SEED, hw=hw)
    aux = synth.clip_inputs(B, Fr, ids, SEED, ragged=True, with_video=False, num_patches=hw * hw)
    return model, feats.cuda(), _kw(aux)


def _step(model, feats_d, kw, B):
    """One forward + backward from cleared gradients -> (logits, {name: grad}, dfeatures)."""
    for p in model.parameters():
        p.grad = None
    x = feats_d.detach().requires_grad_(True)
    out = model(x, **kw)
    (out * _weights(B).cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}, x.grad.clone()


def _check_against_oracle(tag, got, ref, tol):
    (out, grads, dx), (rgrads, rdx, rout) = got, ref
    _close(out, rout, REL_TOL, f"{tag} logits")
    _close(dx, rdx, tol, f"{tag} dfeatures")
    for k, gk in grads.items():
        if float(rgrads[k].abs().max()) == 0.0:
            assert float(gk.abs().max()) == 0.0, f"{tag}: grad {k} is exactly zero in the oracle"
        else:
            _close(gk, rgrads[k], tol, f"{tag} grad {k}")


MODEL_CASES = [(2, 8, 1280, 1, 2),       # one patch per slot: the factored cls hand-over does not fit (fp32 path: 18 token rows)
               (64, 8, 1280, 1, 2),      # ... with 576 token rows, enough for the engine to take the plane path, where the hand-over lives
               (2, 8, 1280, 4, 2),
               (2, 8, 1280, 8, 2),
               (1, 16, 2048, 10, 3),     # the Xception-at-299 geometry
               (1, 32, 1280, 2, 3)]


@pytest.mark.parametrize("B,Fr,C,hw,ids", MODEL_CASES)
def test_backward_all_parameters_vs_oracle(B, Fr, C, hw, ids):
    """Every parameter gradient and dfeatures against torch autograd over oracle.tsf_forward; a gradient that is exactly zero in the
    oracle (the dead rows of the embedding tables) is exactly zero here."""
    model, feats_d, kw = _model_and_inputs(B, Fr, C, hw, ids)
    _check_against_oracle(f"B{B} F{Fr} C{C} hw{hw}", _step(model, feats_d, kw, B), _oracle(B, Fr, C, hw, ids), REL_TOL)


P64 = (2, 8, 1280, 8, 2)


def test_p64_on_the_fp32_mfma_pipe():
    """mt_gemm_set_split(0): fp32 MFMA contractions everywhere, so the engine's fp32 (non-plane) path at 1026 token rows."""
    model, feats_d, kw = _model_and_inputs(*P64)
    prev = L.set_gemm_split(False)
    try:
        got = _step(model, feats_d, kw, P64[0])
    finally:
        L.set_gemm_split(prev)
    _check_against_oracle("p64 split 0", got, _oracle(*P64), REL_TOL)


def test_p64_at_matmul_precision_high():
    import mintime_amd
    model, feats_d, kw = _model_and_inputs(*P64)
    try:
        with mintime_amd.matmul_precision("high"):
            got = _step(model, feats_d, kw, P64[0])
    finally:
        L.set_matmul_precision("highest")
    _check_against_oracle("p64 high", got, _oracle(*P64), TSF_HIGH_GRAD_TOL)


def test_p64_recorded_plan_replays_and_equals_the_eager_step():
    """Consecutive training steps on the same inputs: the first is eager, the second records the launch plan, the third replays it; each
    agrees with the oracle and with the first, and so does a step with the plans switched off (MT_PLAN=0)."""
    from mintime_amd import plans
    model, feats_d, kw = _model_and_inputs(*P64)
    prev = plans.ENABLED
    try:
        plans.ENABLED = True
        first = _step(model, feats_d, kw, P64[0])
        _check_against_oracle("p64 step 1", first, _oracle(*P64), REL_TOL)
        replayed = plans.STATS["replayed"]
        for i in (2, 3):
            got = _step(model, feats_d, kw, P64[0])
            _check_against_oracle(f"p64 step {i}", got, _oracle(*P64), REL_TOL)
            _check_against_oracle(f"p64 step {i} vs step 1", got, (first[1], first[2], first[0]), REL_TOL)
        assert plans.STATS["replayed"] > replayed, "the third step must replay the recorded plans"
        plans.ENABLED = False
        eager = _step(model, feats_d, kw, P64[0])
        _check_against_oracle("p64 plans off vs step 1", eager, (first[1], first[2], first[0]), REL_TOL)
    finally:
        plans.ENABLED = prev


def test_two_patch_counts_alternate_in_one_process():
    """Models at n = 16 and n = 64 take turns (three steps each: eager, recording, replay): no launch plan, workspace or cache of one
    serves the other -- every step gives the values of that model run on its own."""
    from mintime_amd import plans
    cases = [(2, 8, 1280, 4, 2), P64]
    alone = []
    for c in cases:
        model, feats_d, kw = _model_and_inputs(*c)
        alone.append(_step(model, feats_d, kw, c[0]))
        _check_against_oracle(f"hw{c[3]} alone", alone[-1], _oracle(*c), REL_TOL)
    prev = plans.ENABLED
    try:
        plans.ENABLED = True
        live = [_model_and_inputs(*c) for c in cases]
        for step in range(3):
            for c, (model, feats_d, kw), ref in zip(cases, live, alone):
                got = _step(model, feats_d, kw, c[0])
                _check_against_oracle(f"hw{c[3]} alternating, step {step + 1}", got, (ref[1], ref[2], ref[0]), REL_TOL)
    finally:
        plans.ENABLED = prev


@pytest.mark.parametrize("hw", [4, 8])
def test_attention_aggregation_at_other_patch_counts(hw):
    B, Fr, C, ids = 2, 8, 1280, 2
    model, _ = _build(_cfg(C, Fr, hw), SEED, require_attention=True)
    feats = synth.features(B, Fr, C, SEED, hw=hw)
    aux = synth.clip_inputs(B, Fr, ids, SEED, ragged=True, with_video=False, num_patches=hw * hw)
    with torch.no_grad():
        _, (s_att, t_att) = model(feats.cuda(), **_kw(aux))
    assert s_att.shape == (B * HEADS, 1, 1 + Fr * hw * hw) and t_att.shape == s_att.shape
    fpi = [4, 8]
    got, got_id = harness.aggregate_attentions([s_att, t_att], HEADS, Fr, fpi, scale_factor=50000)
    want, want_id = O.aggregate_attentions([s_att.cpu(), t_att.cpu()], HEADS, Fr, fpi, scale_factor=50000)
    _close(torch.tensor(got), torch.tensor(want), REL_TOL, f"hw{hw} aggregated attentions")
    _close(torch.tensor(got_id), torch.tensor(want_id), REL_TOL, f"hw{hw} identity attentions")


def test_train_step_through_the_extractor_at_256():
    """EfficientNet-B0 at 256 x 256 (8 x 8 feature map) feeding a TimeSformer at num-patches 64: the extractor's features against
    oracle.effnet_b0_forward first, then one harness.train_step against oracle.clip_forward + autograd in fp64."""
    from mintime_amd import EfficientNet
    B, Fr, seed = 2, 8, 3
    cfg = arch.default_tsf_config(1280, Fr, num_patches=64, image_size=256)
    ef = EfficientNet.from_name("efficientnet-b0", image_size=256, drop_connect_rate=0.0)
    ef.load_state_dict(synth.effnet_b0_state(seed))
    tsf, _ = _build(cfg, seed)
    ef.cuda().train()
    tsf.train()
    inp = synth.clip_inputs(B, Fr, 2, seed, ragged=True, image_size=256, num_patches=64)
    batch = {k: (v.cuda() if k != "size_embedding" else v) for k, v in inp.items()}
    ef_sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v)
             for k, v in O.to_dtype(synth.effnet_b0_state(seed), torch.float64).items()}
    ts_sd = {k: v.clone().requires_grad_(True) for k, v in O.to_dtype(synth.tsf_state(cfg, seed), torch.float64).items()}
    inp64 = dict(inp)
    inp64["videos"] = inp["videos"].double()
    taps = {}
    yo = O.clip_forward(ef_sd, ts_sd, cfg, inp64, training_extractor=True, taps=taps)
    lo = O.bce_with_logits(yo, inp["labels"])
    lo.backward()
    # the extractor alone (never run at this size before): [B F, 1280, 8, 8]
    v = batch["videos"]
    with torch.no_grad():
        feats = ef(v.reshape(B * Fr, 256, 256, 3).permute(0, 3, 1, 2))
    assert feats.shape == (B * Fr, 1280, 8, 8)
    _close(feats, taps["features"].detach(), REL_TOL, "EfficientNet-B0 features at 256 x 256")
    opt = harness.make_optimizer(cfg, ef, tsf)
    loss = harness.train_step(ef, tsf, opt, batch)
    torch.cuda.synchronize()
    _close(loss, lo.detach(), REL_TOL, "loss")
    for k, p in tsf.named_parameters():
        ref = ts_sd[k].grad
        if float(ref.abs().max()) == 0.0:
            assert float(p.grad.abs().max()) == 0.0, k
        else:
            _close(p.grad, ref, REL_TOL, "grad tsf." + k)
    for k, p in ef.named_parameters():
        if k.startswith("_fc") or k.endswith("_bn2.bias"):       # unused by the forward / analytically zero behind a train-mode BatchNorm
            continue
        _close(p.grad, ef_sd[k].grad, REL_TOL, "grad ef." + k)
