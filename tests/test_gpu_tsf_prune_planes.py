"""The last TimeSformer layer with its dead rows pruned on the plane-operand path (tsf_planes.py).

Part 1, the two entry points the pruned backward needs, through the C ABI on NaN / canary pre-filled buffers, EXACT against the pieces
that already exist (values compared, so +0 and -0 count as equal):
  mt_attn_bwd_cls_planes             == mt_split_planes_blk( mt_attn_bwd mode 2 into a zero-filled fp32 dqkv ), padding rows included
  mt_layernorm_bwd_rows_sums_sparse  == mt_layernorm_bwd_rows_sums fed a dense residual that is zero off the rows r % period == 0
Part 2, the model: pruned (MT_TSF_PRUNE_LAST=1 at small batches; the default from tsf_planes.PRUNE_MIN_CLIPS clips up) against
MT_TSF_PRUNE_LAST=0 (full rows) at the gates of
tests/test_gpu_tsf.py::test_last_layer_dead_row_pruning_is_exact (1e-5 logits / 2e-5 feature gradient / 5e-5 parameter gradients)."""
import pytest
import torch

from mintime_amd import SizeInvariantTimeSformer, arch, plans, synth
from mintime_amd import lib as L

from . import test_gpu_tsf_ops as TO
from . import test_gpu_tsf_patches as TP
from . import tsf_ref as R
from .util import assert_close, rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
DH = 64
SCALE = DH ** -0.5
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3          # csrc/common.hpp
NAN = float("nan")


def _d(t):
    return t.contiguous().to(dev)


# ---- 1a. the cls query's adjoint with plane output ----------------------------------------------------------------------------

def _guarded_planes(rows, cols, fill=NAN):
    """A plane tensor holding `fill` between two 64-element guard bands of -0.0 (any store outside the tensor shows)."""
    shape = L.planes_shape(rows, cols)
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 128,), -0.0, dtype=torch.bfloat16, device=dev)
    body = buf[64:64 + numel]
    body.fill_(fill)
    return buf, body.view(shape)


def _bands_intact(buf):
    bits = buf.view(torch.int16)
    return bool((bits[:64] == -2 ** 15).all() and (bits[-64:] == -2 ** 15).all())


def _cls_planes(qkv_d, dout_d, mask_d, n, B, H, F, fill=NAN, offset_bytes=0):
    """-> (return code, plane tensor) of one mt_attn_bwd_cls_planes call."""
    N, inner = 1 + F * max(n, 1), H * DH
    buf, dp = _guarded_planes(B * N, 3 * inner, fill)
    rc = L.get().mt_attn_bwd_cls_planes(L.ptr(qkv_d), L.ptr(dout_d), L.ptr(mask_d), B, H, F, n, SCALE, dp.data_ptr() + offset_bytes,
                                        L.stream_ptr())
    torch.cuda.synchronize()
    assert _bands_intact(buf), "mt_attn_bwd_cls_planes wrote outside the plane tensor"
    return rc, dp


def _mode2_then_split(qkv_d, dout_d, mask_d, ident_d, n, B, H, F):
    """The existing pieces: mt_attn_bwd mode 2 into a zero-filled dqkv, then mt_split_planes_blk of that tensor."""
    N, inner = 1 + F * n, H * DH
    dqkv = torch.zeros(B * N, 3 * inner, device=dev)
    L.check(L.get().mt_attn_bwd(L.ptr(qkv_d), L.ptr(dout_d), L.ptr(dqkv), L.ptr(mask_d), L.ptr(ident_d), B, H, F, n, 2, SCALE, None,
                                L.stream_ptr()), "mt_attn_bwd mode 2")
    return dqkv, L.split_planes_blk(dqkv, B * N, 3 * inner)


def _decode(planes, cols):
    """fp32 P0 + P1 + P2 of every row of the plane tensor, the padding rows included."""
    return L.planes_to_float(planes, planes.shape[1] * 32, cols)


# (n, B, H, F, mask kind)
CLS_CASES = [(1, 3, 8, 8, "ragged"),        # the smallest clip: N = 9, B N = 27 (no multiple of 32: five padding rows); H = 8
             (49, 1, 1, 8, "ragged"),       # one clip, H = 1; N = 393
             (49, 1, 1, 8, "ones"),
             (7, 2, 8, 16, "zeroclip"),     # F = 16; the second clip's mask is all zero
             (7, 2, 2, 16, "ragged"),
             (100, 2, 2, 8, "ragged"),      # the upper end of n: N = 801, two trips of the 256-key pass and a tail
             (100, 2, 8, 8, "zeroclip")]


@pytest.mark.parametrize("n,B,H,F,kind", CLS_CASES)
def test_cls_adjoint_planes_equal_mode2_then_split(n, B, H, F, kind):
    N, inner = 1 + F * n, H * DH
    qkv, dout, mask, ident, _ = TP._attn_case(n, B, H, F, kind, "moderate")
    qkv_d, dout_d, mask_d, ident_d = _d(qkv), _d(dout), _d(mask.to(torch.uint8)), _d(ident.to(torch.uint8))
    dqkv, ref_p = _mode2_then_split(qkv_d, dout_d, mask_d, ident_d, n, B, H, F)
    rc, dp = _cls_planes(qkv_d, dout_d, mask_d, n, B, H, F)
    L.check(rc, "mt_attn_bwd_cls_planes")
    got, ref = _decode(dp, 3 * inner), _decode(ref_p, 3 * inner)
    assert not bool(torch.isnan(dp.float()).any()), "an element of the plane tensor was not written"
    assert torch.equal(got, ref), f"planes differ from the split of mode 2's dqkv at {int((got != ref).sum())} elements"
    assert torch.equal(got[:B * N], dqkv)                                                # ... which is the fp32 result itself
    assert float(got[B * N:].abs().sum()) == 0.0                                         # padding rows
    patch = torch.ones(B * N, dtype=torch.bool, device=dev)
    patch[::N] = False
    assert float(got[:B * N][patch][:, :inner].abs().sum()) == 0.0                       # dq of the patch rows: exact zeros
    assert float(got[:B * N][~patch][:, :inner].abs().max()) > 0.0                       # dq of the cls rows: written
    # deterministic mode: two runs, the same bits (and the same as the default mode: one block per (clip, head), no atomics)
    prev = L.set_deterministic(True)
    try:
        _, p1 = _cls_planes(qkv_d, dout_d, mask_d, n, B, H, F)
        _, p2 = _cls_planes(qkv_d, dout_d, mask_d, n, B, H, F)
    finally:
        L.set_deterministic(prev)
    assert torch.equal(p1.view(torch.int16), p2.view(torch.int16)) and torch.equal(p1.view(torch.int16), dp.view(torch.int16))


def test_cls_adjoint_planes_without_a_mask_pointer():
    """mask = NULL: nothing is padded (what mt_attn_bwd mode 2 does with a NULL mask)."""
    n, B, H, F = 4, 2, 2, 8
    N, inner = 1 + F * n, H * DH
    qkv, dout, _, _, _ = TP._attn_case(n, B, H, F, "ones", "moderate")
    qkv_d, dout_d = _d(qkv), _d(dout)
    dqkv, ref_p = _mode2_then_split(qkv_d, dout_d, None, None, n, B, H, F)
    rc, dp = _cls_planes(qkv_d, dout_d, None, n, B, H, F)
    L.check(rc, "mt_attn_bwd_cls_planes")
    assert torch.equal(_decode(dp, 3 * inner), _decode(ref_p, 3 * inner))


def test_cls_adjoint_planes_vs_fp64():
    """The data and the gate of tests/test_gpu_tsf_ops.py::test_attention_mode2_is_the_cls_query_alone (the model's own form)."""
    B, H, F, n = 2, 8, 8, TO.n
    N, inner = 1 + F * n, H * DH
    qkv, dout, mask, ident, _ = TO._attn_case(B, H, F, "ragged", "moderate", seed=7)
    dref = R.attn_bwd_ref(qkv.double(), dout.double(), mask, ident, H, F, n, 2, SCALE)
    rc, dp = _cls_planes(_d(qkv), _d(dout), _d(mask.to(torch.uint8)), n, B, H, F)
    L.check(rc, "mt_attn_bwd_cls_planes")
    got = L.planes_to_float(dp, B * N, 3 * inner).reshape(B, N, 3 * inner)
    tol, bad = TO.ATTN_BWD_TOL["moderate"], []
    for name, gt, rf in zip(("dq", "dk", "dv"), got.chunk(3, dim=-1), dref.chunk(3, dim=-1)):
        for rows, sl in (("cls rows", slice(0, 1)), ("patch rows", slice(1, None))):
            if name == "dq" and rows == "patch rows":
                assert float(gt[:, sl].abs().sum()) == 0.0 and float(rf[:, sl].abs().sum()) == 0.0
                continue
            e = rel_err(gt[:, sl], rf[:, sl])
            print(f"FIG cls_planes vs fp64 | {name} {rows} | {e:.3e} | tol {tol:.0e}")
            if not e <= tol:
                bad.append(f"{name} {rows}: {e:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("what", ["n0", "n101", "misaligned", "null"])
def test_cls_adjoint_planes_refusals_write_nothing(what):
    B, H, F = 2, 2, 8
    n = {"n0": 0, "n101": 101}.get(what, 4)
    n_alloc = max(n, 1)
    qkv = torch.randn(B, 1 + F * n_alloc, 3 * H * DH, device=dev)
    dout = torch.randn(B, 1 + F * n_alloc, H * DH, device=dev)
    mask = torch.ones(B, F, dtype=torch.uint8, device=dev)
    if what == "null":
        rc = L.get().mt_attn_bwd_cls_planes(L.ptr(qkv), L.ptr(dout), L.ptr(mask), B, H, F, n, SCALE, None, L.stream_ptr())
        assert rc == MT_ERR_ARG
        return
    N = 1 + F * n_alloc
    buf, dp = _guarded_planes(B * N, 3 * H * DH, 7.0)
    rc = L.get().mt_attn_bwd_cls_planes(L.ptr(qkv), L.ptr(dout), L.ptr(mask), B, H, F, n, SCALE,
                                        dp.data_ptr() + (2 if what == "misaligned" else 0), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == (MT_ERR_ARG if what == "misaligned" else MT_ERR_UNSUPPORTED)
    assert bool((dp == 7.0).all()) and _bands_intact(buf), "a refused call wrote something"


# ---- 1b. LayerNorm backward with a sparse residual ------------------------------------------------------------------------------

def _ln_case(rows, period, D):
    g = torch.Generator().manual_seed(rows * 1000 + D)
    x, dy = torch.randn(rows, D, generator=g) * 1.5 + 0.3, torch.randn(rows, D, generator=g)
    gamma = torch.rand(D, generator=g) + 0.5
    res = torch.randn(rows // period, D, generator=g)
    mean, var = x.double().mean(1), x.double().var(1, unbiased=False)
    stats = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-5)], 1).float()
    return _d(x), _d(dy), _d(gamma), _d(res), _d(stats)


@pytest.mark.parametrize("skip_is_period", [False, True], ids=["skip0", "skip_period"])
@pytest.mark.parametrize("D", [512, 64])
@pytest.mark.parametrize("rows,period", [(27, 9), (786, 393)])       # a partial 32-row block; two clips of the model's own length
def test_sparse_residual_layernorm_backward_equals_the_dense_form(rows, period, D, skip_is_period):
    lib = L.get()
    skip = period if skip_is_period else 0
    x, dy, gamma, res, stats = _ln_case(rows, period, D)
    dense = torch.zeros(rows, D, device=dev)
    dense[::period] = res
    nb = lib.mt_layernorm_bwd_rows_blocks(rows)
    outs = []
    for sparse in (False, True):
        dx = torch.full((rows, D), NAN, device=dev)
        part = torch.full((nb, 3, D), NAN, device=dev)
        buf, dxp = _guarded_planes(rows, D)
        if sparse:
            L.check(lib.mt_layernorm_bwd_rows_sums_sparse(L.ptr(dy), L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(dx), L.ptr(res), period,
                                                          rows, D, L.ptr(dxp), L.ptr(part), skip, L.stream_ptr()), "ln bwd sparse")
        else:
            L.check(lib.mt_layernorm_bwd_rows_sums(L.ptr(dy), L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(dx), L.ptr(dense), rows, D,
                                                   L.ptr(dxp), L.ptr(part), skip, L.stream_ptr()), "ln bwd dense")
        torch.cuda.synchronize()
        assert _bands_intact(buf)
        outs.append((dx, _decode(dxp, D), part))
    (dx0, p0, s0), (dx1, p1, s1) = outs
    for t in (dx1, p1, s1):
        assert not bool(torch.isnan(t).any()), "an output element was not written"
    assert torch.equal(dx1, dx0) and torch.equal(p1, p0) and torch.equal(s1, s0)
    assert float(p1[rows:].abs().sum()) == 0.0 and torch.equal(p1[:rows], dx1)
    # and the residual did arrive: the cls rows differ from LN'(dy) alone by res
    dx_plain, zero, part2 = torch.full((rows, D), NAN, device=dev), torch.zeros_like(dense), torch.empty_like(s0)
    L.check(lib.mt_layernorm_bwd_rows_sums(L.ptr(dy), L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(dx_plain), L.ptr(zero), rows, D, None,
                                           L.ptr(part2), skip, L.stream_ptr()), "ln bwd plain")
    keep = torch.ones(rows, dtype=torch.bool, device=dev)
    keep[::period] = False
    assert torch.equal(dx1[keep], dx_plain[keep])
    # (two fp32 roundings of values of size <= ~10 against max |res| ~ 4: a few 1e-7)
    assert_close(dx1[~keep] - dx_plain[~keep], res, 1e-5, "residual on the cls rows")


def test_sparse_residual_layernorm_backward_refusals():
    lib = L.get()
    x, dy, gamma, res, stats = _ln_case(27, 9, 64)
    dx = torch.full((27, 64), 7.0, device=dev)
    part = torch.full((lib.mt_layernorm_bwd_rows_blocks(27), 3, 64), 7.0, device=dev)
    for period, D in ((10, 64), (0, 64)):                      # rows no multiple of the period; no period
        rc = lib.mt_layernorm_bwd_rows_sums_sparse(L.ptr(dy), L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(dx), L.ptr(res), period, 27, D,
                                                   None, L.ptr(part), 0, L.stream_ptr())
        assert rc == MT_ERR_ARG
    rc = lib.mt_layernorm_bwd_rows_sums_sparse(L.ptr(dy), L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(dx), L.ptr(res), 9, 27, 516, None,
                                               L.ptr(part), 0, L.stream_ptr())
    assert rc == MT_ERR_UNSUPPORTED                            # dim <= 512 like the dense form
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((part == 7.0).all())


# ---- 2. the model ------------------------------------------------------------------------------------------------------------------

C = 1280


def _build(cfg, seed, require_attention=True):
    model = SizeInvariantTimeSformer(config=cfg, require_attention=require_attention)
    model.load_state_dict(synth.tsf_state(cfg, seed), strict=True)
    return model.cuda()


def _case(B, Fr, ids, ragged, seed=9):
    feats = synth.features(B, Fr, C, seed)
    aux = synth.clip_inputs(B, Fr, ids, seed, ragged=ragged, with_video=False)
    kw = dict(mask=aux["mask"].cuda(), identities_mask=aux["identities_mask"].cuda(), size_embedding=aux["size_embedding"],
              positions=aux["positions"].cuda())
    return feats, aux, kw


def _set_prune(monkeypatch, flag):
    if flag is None:
        monkeypatch.delenv("MT_TSF_PRUNE_LAST", raising=False)
    else:
        monkeypatch.setenv("MT_TSF_PRUNE_LAST", flag)


def _train_step(model, feats, aux, kw, expect_pruned):
    """One forward + backward; -> (logits, space map, time map, feature gradient, {name: parameter gradient})."""
    for p in model.parameters():
        p.grad = None
    x = feats.cuda().requires_grad_(True)
    out = model(x, **kw)
    logits, (s_att, t_att) = out if model.require_attention else (out, (None, None))
    saved = logits.grad_fn.saved
    assert saved["planes"] and bool(saved.get("pruned_last")) == expect_pruned        # on the plane path, pruned or not as expected
    assert not hasattr(model, "_wT_cache")                                             # (the in-kernel-split engine's cache: never made)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, aux["labels"].reshape(-1, 1).cuda()).backward()
    return logits.detach().clone(), s_att, t_att, x.grad.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _compare(pruned, full, exact_zero_params=True):
    assert_close(pruned[0], full[0], 1e-5, "logits")
    if pruned[1] is not None:
        assert torch.equal(pruned[1], full[1]) and torch.equal(pruned[2], full[2])      # same cls kernels, same inputs
    assert_close(pruned[3], full[3], 2e-5, "feature gradient")
    assert pruned[4].keys() == full[4].keys()
    for k, g in full[4].items():
        if float(g.abs().max()) == 0.0:
            assert float(pruned[4][k].abs().max()) == 0.0, k
        else:
            assert_close(pruned[4][k], g, 5e-5, "grad " + k)


@pytest.mark.parametrize("B,Fr,ids,ragged", [(2, 8, 2, True), (3, 16, 3, False)])
def test_pruned_equals_full_rows(B, Fr, ids, ragged, monkeypatch):
    cfg = arch.default_tsf_config(C, Fr)
    feats, aux, kw = _case(B, Fr, ids, ragged)
    assert B * (1 + Fr * 49) >= 512
    runs = {}
    for flag in ("0", "1"):
        _set_prune(monkeypatch, flag)
        runs[flag] = _train_step(_build(cfg, 9), feats, aux, kw, expect_pruned=flag == "1")
    _compare(runs["1"], runs["0"])
    _set_prune(monkeypatch, None)                                                       # unset, below PRUNE_MIN_CLIPS clips: full rows
    unset = _train_step(_build(cfg, 9), feats, aux, kw, expect_pruned=False)
    assert torch.equal(unset[0], runs["0"][0])


def test_default_prunes_from_32_clips_and_equals_full_rows(monkeypatch):
    """The default (switch unset) at the smallest batch that prunes by default; depth 1 keeps the case small."""
    from mintime_amd import tsf_planes
    B = tsf_planes.PRUNE_MIN_CLIPS
    cfg = arch.default_tsf_config(C, 8)
    cfg["model"]["depth"] = 1
    feats, aux, kw = _case(B, 8, 2, True)
    runs = {}
    for flag in ("0", None):
        _set_prune(monkeypatch, flag)
        runs[flag] = _train_step(_build(cfg, 9), feats, aux, kw, expect_pruned=flag is None)
    _compare(runs[None], runs["0"])


def test_depth_one(monkeypatch):
    """The last layer is also the first: its time attention's LayerNorm backward feeds the patch embedding's bias sum (skip = N)."""
    cfg = arch.default_tsf_config(C, 8)
    cfg["model"]["depth"] = 1
    feats, aux, kw = _case(2, 8, 2, True)
    runs = {}
    for flag in ("0", "1"):
        _set_prune(monkeypatch, flag)
        runs[flag] = _train_step(_build(cfg, 9), feats, aux, kw, expect_pruned=flag == "1")
    _compare(runs["1"], runs["0"])
    assert float(runs["1"][4]["to_patch_embedding.bias"].abs().max()) > 0.0


def test_eval_forward_without_grad(monkeypatch):
    cfg = arch.default_tsf_config(C, 8)
    feats, aux, kw = _case(2, 8, 2, True)
    outs = {}
    for flag in ("0", "1"):
        _set_prune(monkeypatch, flag)
        model = _build(cfg, 9).eval()
        with torch.no_grad():
            logits, (s_att, t_att) = model(feats.cuda(), **kw)
        outs[flag] = (logits, s_att, t_att)
    assert_close(outs["1"][0], outs["0"][0], 1e-5, "eval logits")
    assert torch.equal(outs["1"][1], outs["0"][1]) and torch.equal(outs["1"][2], outs["0"][2])


def test_three_steps_eager_recorded_replayed_are_bit_identical(monkeypatch):
    """One model, unchanged weights, deterministic mode: the first step runs eagerly, the second records the launch plans, the third
    replays them -- the pruned phase holds library calls only, so it records, and every step gives the same bits."""
    _set_prune(monkeypatch, "1")
    cfg = arch.default_tsf_config(C, 8)
    cfg["model"]["depth"] = 2
    feats, aux, kw = _case(2, 8, 2, True)
    model = _build(cfg, 9)
    prev_det, prev_plans = L.set_deterministic(True), plans.ENABLED
    try:
        plans.ENABLED = True
        recorded, replayed = plans.STATS["recorded"], plans.STATS["replayed"]
        eager = _train_step(model, feats, aux, kw, expect_pruned=True)
        assert plans.STATS["recorded"] == recorded and plans.STATS["replayed"] == replayed
        rec = _train_step(model, feats, aux, kw, expect_pruned=True)
        assert plans.STATS["recorded"] == recorded + 1 and plans.STATS["replayed"] == replayed
        rep = _train_step(model, feats, aux, kw, expect_pruned=True)
        assert plans.STATS["replayed"] == replayed + 2, "the third step must replay the forward and the backward plan"
    finally:
        plans.ENABLED = prev_plans
        L.set_deterministic(prev_det)
    for step in (rec, rep):
        assert torch.equal(step[0], eager[0]) and torch.equal(step[1], eager[1]) and torch.equal(step[2], eager[2])
        assert torch.equal(step[3], eager[3]), "feature gradient"
        for k, g in eager[4].items():
            assert torch.equal(step[4][k], g), k


def test_ff_dropout_keeps_full_rows(monkeypatch):
    """The reference draws a dropout's multipliers in the shape of ALL rows: with a dropout active the last layer is not pruned, and the
    step is the one MT_TSF_PRUNE_LAST=0 gives for the same draws -- also when the switch asks for pruning."""
    cfg = arch.default_tsf_config(C, 8)
    cfg["model"]["depth"], cfg["model"]["ff-dropout"] = 2, 0.1
    feats, aux, kw = _case(2, 8, 2, True)
    runs = {}
    prev = L.set_deterministic(True)            # (fixed summation orders: the two runs are the same launches, so the same bits)
    try:
        for flag in ("0", "1"):
            _set_prune(monkeypatch, flag)
            model = _build(cfg, 9, require_attention=False).train()
            calls = []

            def sampler(shape, device, calls=calls):
                calls.append(tuple(shape))
                return torch.rand(shape, generator=torch.Generator().manual_seed(100 + len(calls))).to(device)

            model.dropout_uniform = sampler
            runs[flag] = _train_step(model, feats, aux, kw, expect_pruned=False)
            assert calls == [(2 * 393, 4 * cfg["model"]["dim"])] * 2                    # one draw per layer, all rows
    finally:
        L.set_deterministic(prev)
    a, b = runs["1"], runs["0"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    for k, g in b[4].items():
        assert torch.equal(a[4][k], g), k
