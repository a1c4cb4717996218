"""GPU tests of the matmul precision tier "high" (include/mintime_hip.h: mt_gemm_set_precision): three piece products
a0 b0 + a0 b1 + a1 b0 of the exact bf16 split instead of six, on the plane-operand loop (mt_gemm_planes) and on mt_gemm's
split-operand loop.  Kernel level: crafted operands whose results tell the tiers apart exactly, random operands against the tier's
own arithmetic (fp64 sum of the three piece products) and against fp64 within the tier's error bound, the stream-K / persistent /
deterministic variants.  Model level: the TimeSformer and EfficientNet fixtures at the project's output tolerance, launch plans."""
import math

import pytest
import torch

import mintime_amd
from mintime_amd import arch, harness, optim, plans, synth, EfficientNet, SizeInvariantTimeSformer
from mintime_amd import lib as L
from oracle import mintime_oracle as O
from tests.util import REL_TOL, assert_close, golden, rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5                         # tests/test_gpu_planes.py: the plane loop against its own exact sum

# Gradient gates at tier high.  The rule: 2x the worst rel_err against the reference's fp64 values measured on an MI355X over the whole
# set of comparisons of the test that uses them (the habit of tests/test_gpu_e2e.py), never above REL_TOL.  Measured
# (profiles/precision_high_step.txt):
#   TimeSformer, 4 fixtures x 18 slices: worst 5.385e-4 (tsf_cfg1, gslice.layers.4.2.fn.net.0.weight); the other fixtures 2.2e-4 .. 3.7e-4.
#     2 x 5.385e-4 = 1.077e-3 is above the cap, so the gate is the cap.
#   EfficientNet-B0, 16 crops, 195 parameter gradients: worst 1.738e-4 (_blocks.8._se_reduce.bias); gate 2 x 1.738e-4.
TSF_HIGH_GRAD_TOL = min(2 * 5.385e-4, REL_TOL)
EF_HIGH_GRAD_TOL = min(2 * 1.738e-4, REL_TOL)


@pytest.fixture(autouse=True)
def _restore_highest():
    try:
        yield
    finally:
        L.set_matmul_precision("highest")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _pieces(x):
    """The first two pieces of the exact split (round-to-nearest bf16 at each level), as fp64."""
    p0 = x.bfloat16().float()
    p1 = (x - p0).bfloat16().float()
    return p0.double(), p1.double()


def _h(A, B):
    """The tier's own arithmetic for C = A . B (A [M, K], B [K, N]) in fp64: a0 b0 + a0 b1 + a1 b0."""
    a0, a1 = _pieces(A)
    b0, b1 = _pieces(B)
    return a0 @ b0 + a0 @ b1 + a1 @ b0


def _envelope_ok(got, exact, absprod, K, what):
    """Check 2: |C - A.B| <= (3.1 * 2^-16 + (K / 16 + 4) * 2^-23) * (|A| . |B|) element-wise.  First term: the dropped products
    a1 b1 + a r_b + r_a b with |x - x0| <= 2^-8 |x|, |x - x0 - x1| <= 2^-16 |x|; second: fp32 accumulation over K / 16 MFMA steps
    plus the accumulator pair."""
    bound = (3.1 * 2.0 ** -16 + (K / 16 + 4) * 2.0 ** -23) * absprod
    err = (got.detach().cpu().double() - exact).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"[precision] {what}: worst |err| / envelope = {worst:.3f}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the tier's envelope"


def _planes_gemm(op, A, B, M, N, K, **kw):
    """mt_gemm_planes on fp32 host operands as stored (A [M,K] or [K,M] for TN; B [N,K] for NT, [K,N] otherwise)."""
    out = torch.zeros(M, N, device="cuda") if op == L.OP_TN else torch.full((M, N), float("nan"), device="cuda")
    if op == L.OP_TN:
        kw.setdefault("epilogue", L.EPI_ATOMIC)
    kw.setdefault("streamk", False)
    L.gemm_planes(op, L.split_planes_blk(A.cuda()), L.split_planes_blk(B.cuda()), M, N, K, Cout=out, ldc=N, **kw)
    return out


# ---- (a) tier discrimination on crafted operands -----------------------------------------------------------------------------
U = 1.0 + 2.0 ** -9 + 2.0 ** -18          # splits as (1, 2^-9, 2^-18)
V = 1.0 + 2.0 ** -9                       # splits as (1, 2^-9, 0)

CRAFTED = [("planes", L.OP_NT, 129, 128, 16), ("planes", L.OP_NT, 300, 192, 136), ("planes", L.OP_NN, 300, 136, 512),
           ("planes", L.OP_TN, 136, 200, 1179), ("gemm", L.OP_NT, 786, 1536, 512)]


@pytest.mark.parametrize("path,op,M,N,K", CRAFTED)
@pytest.mark.parametrize("case", ["a_is_u", "b_is_u", "both_v"])
def test_crafted_operands_tell_the_tiers_apart(path, op, M, N, K, case):
    """Every product is exact in fp32, so the expected values are derived, not measured: with A = u, B = 1 the six-product tier
    gives K u and the three-product tier K (1 + 2^-9) (a2 b0 = 2^-18 is dropped); with A = B = 1 + 2^-9 highest keeps
    a1 b1 = 2^-18 and high drops it.  The two targets lie K 2^-18 apart and each is gated at K 2^-20."""
    assert torch.tensor(U).bfloat16().item() == 1.0 and (torch.tensor(U) - 1.0).bfloat16().item() == 2.0 ** -9
    assert float(torch.tensor(U) - 1.0 - 2.0 ** -9) == 2.0 ** -18
    va, vb = {"a_is_u": (U, 1.0), "b_is_u": (1.0, U), "both_v": (V, V)}[case]
    want = {"a_is_u": {"highest": K * U, "high": K * V}, "b_is_u": {"highest": K * U, "high": K * V},
            "both_v": {"highest": K * (1 + 2.0 ** -8 + 2.0 ** -18), "high": K * (1 + 2.0 ** -8)}}[case]
    a_shape = (K, M) if op == L.OP_TN else (M, K)
    b_shape = (N, K) if op == L.OP_NT else (K, N)
    A, B = torch.full(a_shape, va), torch.full(b_shape, vb)
    tol = K * 2.0 ** -20
    got = {}
    for tier in ("highest", "high"):
        L.set_matmul_precision(tier)
        if path == "planes":
            c = _planes_gemm(op, A, B, M, N, K)
        else:
            c = torch.full((M, N), float("nan"), device="cuda")
            prev = L.set_gemm_split(True)
            try:
                L.gemm(op, A.cuda(), B.cuda(), c, M, N, K, K, K, N)
            finally:
                L.set_gemm_split(prev)
        got[tier] = c.cpu().double()
    L.set_matmul_precision("highest")
    for tier, other in (("highest", "high"), ("high", "highest")):
        worst = float((got[tier] - want[tier]).abs().max())
        assert worst <= tol, f"{tier}: |C - {want[tier]!r}| = {worst:.3e} > K 2^-20 = {tol:.3e}"
        miss = float((got[tier] - want[other]).abs().min())
        assert miss > tol, f"{tier} also meets the {other} target: the tiers are not distinguished"


# ---- (b) random operands: the tier's own arithmetic, and fp64 within the tier's envelope ------------------------------------------
@pytest.mark.parametrize("M,N,K,res", [(129, 128, 16, False), (300, 192, 136, False), (786, 1536, 512, False), (786, 1536, 512, True)])
def test_nt_at_high(M, N, K, res):
    A, W, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.05), _rand(N, seed=3)
    R = _rand(M, N, seed=5) if res else None
    L.set_matmul_precision("high")
    kw = dict(bias=b.cuda())
    if res:
        kw.update(epilogue=L.EPI_BIAS_RES, R=R.cuda(), ldr=N)
    got = _planes_gemm(L.OP_NT, A, W, M, N, K, **kw)
    L.set_matmul_precision("highest")
    extra = b.double() + (R.double() if res else 0.0)
    assert_close(got, _h(A, W.T) + extra, TOL, "NT at high vs its own arithmetic")
    _envelope_ok(got, A.double() @ W.double().T + extra, A.double().abs() @ W.double().abs().T, K, f"NT {M} x {N} x {K}")


@pytest.mark.parametrize("M,N,K", [(300, 136, 512), (786, 512, 520)])
def test_nn_at_high(M, N, K):
    dY, W = _rand(M, K, seed=1), _rand(K, N, seed=2, scale=0.05)
    L.set_matmul_precision("high")
    got = _planes_gemm(L.OP_NN, dY, W, M, N, K)
    L.set_matmul_precision("highest")
    assert_close(got, _h(dY, W), TOL, "NN at high vs its own arithmetic")
    _envelope_ok(got, dY.double() @ W.double(), dY.double().abs() @ W.double().abs(), K, f"NN {M} x {N} x {K}")


@pytest.mark.parametrize("Mo,No,K", [(136, 200, 1179), (1536, 512, 786)])
def test_tn_at_high(Mo, No, K):
    dY, X = _rand(K, Mo, seed=1, scale=0.1), _rand(K, No, seed=2)
    L.set_matmul_precision("high")
    got = _planes_gemm(L.OP_TN, dY, X, Mo, No, K)
    L.set_matmul_precision("highest")
    assert_close(got, _h(dY.T, X), TOL, "TN at high vs its own arithmetic")
    _envelope_ok(got, dY.double().T @ X.double(), dY.double().abs().T @ X.double().abs(), K, f"TN {Mo} x {No} x {K}")


def test_stats_epilogue_at_high():
    M, N, K = 1000, 728, 728
    a, w = _rand(M, K, seed=4), _rand(N, K, seed=5, scale=0.05)
    ap, wp = L.split_planes_blk(a.cuda()), L.split_planes_blk(w.cuda())
    slots = 32
    out = torch.full((M, N), float("nan"), device="cuda")
    stats = torch.zeros(slots, 2, N, dtype=torch.float64, device="cuda")
    L.set_matmul_precision("high")
    L.gemm_planes(L.OP_NT, ap, wp, M, N, K, Cout=out, ldc=N, epilogue=L.EPI_STATS, stats=stats, stats_slots=slots)
    L.set_matmul_precision("highest")
    assert_close(out, _h(a, w.T), TOL, "STATS at high vs its own arithmetic")
    _envelope_ok(out, a.double() @ w.double().T, a.double().abs() @ w.double().abs().T, K, "STATS 1000 x 728 x 728")
    s = stats.sum(0)
    assert_close(s[0], out.double().sum(0), 1e-6, "column sums")
    assert_close(s[1], (out.double() ** 2).sum(0), 1e-6, "column sums of squares")


def _gelu64(g):
    cdf = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
    return g * cdf, cdf + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def test_geglu_pair_at_high():
    """FF1 with the GEGLU epilogue (fp32 h and plane h) and the GEGLU backward behind FF2's data gradient, at M = 786."""
    M, D = 786, 512
    A, W, b = _rand(M, D, seed=1), _rand(8 * D, D, seed=2, scale=0.05), _rand(8 * D, seed=3, scale=0.1)
    a_p, w_p, bd = L.split_planes_blk(A.cuda()), L.split_planes_blk(W.cuda()), b.cuda()
    L.set_matmul_precision("high")
    h_p = L.planes_empty(M, 4 * D, "cuda")
    h_p.fill_(float("nan"))
    u = torch.full((M, 8 * D), float("nan"), device="cuda")
    L.gemm_planes(L.OP_NT, a_p, w_p, M, 8 * D, D, epilogue=L.EPI_GEGLU, bias=bd, C2=u, ldc2=8 * D, n_half=4 * D, c_planes=h_p, streamk=False)
    h32 = torch.full((M, 4 * D), float("nan"), device="cuda")
    u32 = torch.full((M, 8 * D), float("nan"), device="cuda")
    L.gemm_planes(L.OP_NT, a_p, w_p, M, 8 * D, D, Cout=h32, ldc=4 * D, epilogue=L.EPI_GEGLU, bias=bd, C2=u32, ldc2=8 * D, n_half=4 * D,
                  streamk=False)
    pre = _h(A, W.T) + b.double()                        # [M, 8 D]: the 'a' half, then the gate half
    u_want = torch.stack([pre[:, :4 * D], pre[:, 4 * D:]], dim=-1).reshape(M, 8 * D)      # stored as (a_0, g_0, a_1, g_1, ...)
    assert_close(u, u_want, TOL, "pre-activations at high vs their own arithmetic")
    assert torch.equal(u32, u), "pre-activations, fp32-output instance"
    assert_close(h32, pre[:, :4 * D] * _gelu64(pre[:, 4 * D:])[0], TOL, "h at high")
    assert torch.equal(L.planes_to_float(h_p, M, 4 * D), h32), "h planes = the exact split of the fp32 h"
    assert not torch.isnan(h_p.float()).any() and float(L.planes_to_float(h_p, h_p.shape[1] * 32, 4 * D)[M:].abs().sum()) == 0.0
    # backward
    dx, W2 = _rand(M, D, seed=7), _rand(D, 4 * D, seed=8, scale=0.05)
    _geglu_bwd_check(M, D, dx, W2, u)


def _geglu_bwd_check(M, D, dx, W2, u):
    dx_p, w2_p = L.split_planes_blk(dx.cuda()), L.split_planes_blk(W2.cuda())
    L.set_matmul_precision("high")
    du_p = L.planes_empty(M, 8 * D, "cuda")
    du_p.fill_(float("nan"))
    du = torch.full((M, 8 * D), float("nan"), device="cuda")
    cs = torch.zeros(8 * D, device="cuda")
    L.gemm_planes(L.OP_NN, dx_p, w2_p, M, 4 * D, D, Cout=du, ldc=8 * D, epilogue=L.EPI_GEGLU_BWD, C2=u, ldc2=8 * D, n_half=4 * D, col_sum=cs,
                  c_planes=du_p, streamk=False)
    du32 = torch.full((M, 8 * D), float("nan"), device="cuda")
    cs32 = torch.zeros(8 * D, device="cuda")
    L.gemm_planes(L.OP_NN, dx_p, w2_p, M, 4 * D, D, Cout=du32, ldc=8 * D, epilogue=L.EPI_GEGLU_BWD, C2=u, ldc2=8 * D, n_half=4 * D,
                  col_sum=cs32, streamk=False)
    L.set_matmul_precision("highest")
    dh = _h(dx, W2)
    u64 = u.cpu().double().reshape(M, 4 * D, 2)
    gl, gr = _gelu64(u64[..., 1])
    want = torch.cat([dh * gl, dh * u64[..., 0] * gr], dim=1)
    assert not torch.isnan(du).any()
    assert_close(du, want, TOL, f"du at high, D = {D}")
    assert_close(du[:, 4 * D:], want[:, 4 * D:], TOL, f"dg half of du at high, D = {D}")
    assert torch.equal(du32, du), "fp32-output instance"
    assert torch.equal(L.planes_to_float(du_p, M, 8 * D), du), "du planes = the exact split of the fp32 du"
    assert float(L.planes_to_float(du_p, du_p.shape[1] * 32, 8 * D)[M:].abs().sum()) == 0.0
    assert_close(cs, du.double().sum(0), 1e-4, "column sums of du")
    assert_close(cs32, du.double().sum(0), 1e-4, "column sums of du, fp32-output instance")


def test_geglu_backward_at_high_when_the_half_width_is_not_a_multiple_of_the_block_tile():
    M, D = 786, 48
    A, W, b = _rand(M, D, seed=1), _rand(8 * D, D, seed=2, scale=0.2), _rand(8 * D, seed=3, scale=0.1)
    u = torch.empty(M, 8 * D, device="cuda")
    h = torch.empty(M, 4 * D, device="cuda")
    L.gemm(L.OP_NT, A.cuda(), W.cuda(), h, M, 8 * D, D, D, D, 4 * D, epilogue=L.EPI_GEGLU, bias=b.cuda(), C2=u, ldc2=8 * D, n_half=4 * D)
    _geglu_bwd_check(M, D, _rand(M, D, seed=7), _rand(D, 4 * D, seed=8, scale=0.2), u)


# ---- (c) variants agree, (d) determinism, (e) the default is untouched ------------------------------------------------------------
VARIANT_SHAPES = [(12576, 1536, 512, L.EPI_STORE), (1000, 512, 2048, L.EPI_BIAS_RES)]


def _variant_operands(M, N, K, epi):
    a_p, b_p = L.split_planes_blk(_rand(M, K, seed=1).cuda()), L.split_planes_blk(_rand(N, K, seed=2, scale=0.05).cuda())
    kw = dict(ldc=N, epilogue=epi, bias=_rand(N, seed=3).cuda())
    if epi == L.EPI_BIAS_RES:
        kw.update(R=_rand(M, N, seed=4).cuda(), ldr=N)
    return a_p, b_p, kw


@pytest.mark.parametrize("M,N,K,epi", VARIANT_SHAPES)
def test_stream_k_at_high_matches_one_block_per_tile_and_is_reproducible(M, N, K, epi):
    a_p, b_p, kw = _variant_operands(M, N, K, epi)
    L.set_matmul_precision("high")
    outs = []
    for sk in (False, True, True):
        c = torch.full((M, N), float("nan"), device="cuda")
        L.gemm_planes(L.OP_NT, a_p, b_p, M, N, K, Cout=c, streamk=sk, **kw)
        outs.append(c)
    L.set_matmul_precision("highest")
    assert_close(outs[1], outs[0], TOL, "stream-K vs one block per tile at high")
    assert torch.equal(outs[1], outs[2]), "stream-K must be bit-reproducible"
    ws = L.streamk_workspace("cuda")
    assert ws is not None and int(ws[:4096].view(torch.int32).abs().sum()) == 0, "flags must be cleared by their consumers"


# (the persistent form is only taken with more tiles than resident block slots, 2 x 256: the second shape keeps one block per tile
# on both runs, so a BIAS_RES shape with 99 x 12 tiles and a ragged K is added to run that instance too)
@pytest.mark.parametrize("M,N,K,epi", VARIANT_SHAPES + [(12576, 1536, 520, L.EPI_BIAS_RES)])
def test_persistent_blocks_at_high_give_the_same_bits(M, N, K, epi):
    a_p, b_p, kw = _variant_operands(M, N, K, epi)
    lib = L.get()
    L.set_matmul_precision("high")
    prev = lib.mt_gemm_planes_set_persist(0)
    outs = []
    try:
        for per_cu in (0, 2):
            lib.mt_gemm_planes_set_persist(per_cu)
            c = torch.full((M, N), float("nan"), device="cuda")
            L.gemm_planes(L.OP_NT, a_p, b_p, M, N, K, Cout=c, streamk=False, **kw)
            outs.append(c)
    finally:
        lib.mt_gemm_planes_set_persist(prev)
        L.set_matmul_precision("highest")
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[1], outs[0])


def test_deterministic_weight_gradient_at_high_is_bit_identical_over_two_runs():
    Mo, No, K = 1536, 512, 786
    dY, X = _rand(K, Mo, seed=1, scale=0.1), _rand(K, No, seed=2)
    prev = L.set_deterministic(True)
    try:
        L.set_matmul_precision("high")
        runs = [_planes_gemm(L.OP_TN, dY, X, Mo, No, K) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        L.set_matmul_precision("highest")
        L.set_deterministic(prev)
    assert torch.equal(runs[0], runs[1])
    assert_close(runs[0], _h(dY.T, X), TOL, "deterministic TN at high vs its own arithmetic")


def test_the_default_tier_is_untouched_by_a_round_trip():
    M, N, K = 786, 1536, 512
    A, W, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.05), _rand(N, seed=3)
    L.set_matmul_precision("highest")
    before = _planes_gemm(L.OP_NT, A, W, M, N, K, bias=b.cuda())
    ref = torch.full((M, N), float("nan"), device="cuda")           # the in-kernel six-product loop: the same bits (test_gpu_planes.py)
    prev = L.set_gemm_split(True)
    try:
        L.gemm(L.OP_NT, A.cuda(), W.cuda(), ref, M, N, K, K, K, N, bias=b.cuda())
    finally:
        L.set_gemm_split(prev)
    assert L.set_matmul_precision("high") == "highest"
    at_high = _planes_gemm(L.OP_NT, A, W, M, N, K, bias=b.cuda())
    assert L.set_matmul_precision("highest") == "high"
    after = _planes_gemm(L.OP_NT, A, W, M, N, K, bias=b.cuda())
    assert torch.equal(after, before) and torch.equal(before, ref)
    assert not torch.equal(at_high, before)


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _tsf(g, require_attention):
    B, Fr, C = int(g["batch"]), int(g["frames"]), int(g["channels"])
    feats = synth.features(B, Fr, C, int(g["seed"]))
    aux = synth.clip_inputs(B, Fr, int(g["identities"]), int(g["seed"]), ragged=bool(g["ragged"]), with_video=False)
    cfg = arch.default_tsf_config(C, Fr)
    if "pos_emb" in g.files:
        cfg["model"]["enable-pos-emb"], cfg["model"]["enable-size-emb"] = bool(g["pos_emb"]), bool(g["size_emb"])
    model = SizeInvariantTimeSformer(config=cfg, require_attention=require_attention)
    model.load_state_dict(synth.tsf_state(cfg, int(g["seed"])), strict=True)
    assert B * (1 + Fr * 49) >= 512, "the plane path needs at least 512 token rows"
    return model.cuda(), feats, aux, Fr


@pytest.mark.parametrize("name", ["tsf_cfg1", "tsf_2id_ragged"])
def test_timesformer_forward_at_high(name):
    g = golden(name)
    model, feats, aux, Fr = _tsf(g, True)
    with torch.no_grad(), mintime_amd.matmul_precision("high"):
        logits, (s_att, t_att) = model(feats.cuda(), mask=aux["mask"].cuda(), identities_mask=aux["identities_mask"].cuda(),
                                       size_embedding=aux["size_embedding"], positions=aux["positions"].cuda())
        torch.cuda.synchronize()
    for what, got, ref in (("logits", logits, g["logits"]), ("space cls attention", s_att, g["space_att"]),
                           ("time cls attention", t_att, g["time_att"])):
        print(f"[precision] {name} {what} at high: rel err {rel_err(got, ref):.3e}")
        assert_close(got, ref, REL_TOL, f"{what} at high vs reference")


@pytest.mark.parametrize("name", ["tsf_cfg1", "tsf_2id_ragged", "tsf_nopos", "tsf_nosize"])
def test_timesformer_backward_at_high(name):
    """Loss and gradient norms at REL_TOL; the 256-element gradient slices and the feature-gradient slice at TSF_HIGH_GRAD_TOL."""
    g = golden(name)
    model, feats, aux, Fr = _tsf(g, False)
    x = feats.cuda().requires_grad_(True)
    with mintime_amd.matmul_precision("high"):
        out = model(x, mask=aux["mask"].cuda(), identities_mask=aux["identities_mask"].cuda(),
                    size_embedding=aux["size_embedding"], positions=aux["positions"].cuda())
        loss = torch.nn.functional.binary_cross_entropy_with_logits(out.cpu(), aux["labels"].reshape(-1, 1))
        loss.backward()
        torch.cuda.synchronize()
    assert_close(loss, g["loss"], REL_TOL, "loss at high")
    named = dict(model.named_parameters())
    slices = []
    for k in g.files:
        if k.startswith("gnorm."):
            key = k[len("gnorm."):]
            assert named[key].grad is not None, key
            assert_close(named[key].grad.norm(), g[k], REL_TOL, k + " at high")
            if "gslice." + key in g.files:
                slices.append(("gslice." + key, rel_err(named[key].grad.reshape(-1)[:256], g["gslice." + key])))
    assert_close(x.grad.norm(), g["dfeats_norm"], REL_TOL, "dfeats norm at high")
    slices.append(("dfeats slice", rel_err(x.grad.permute(0, 1, 3, 4, 2).reshape(-1)[:512], g["dfeats_slice"])))
    worst = max(slices, key=lambda t: t[1])
    print(f"[precision] {name} backward at high: worst slice rel err {worst[1]:.3e} ({worst[0]}) of {len(slices)}")
    assert TSF_HIGH_GRAD_TOL <= REL_TOL
    assert worst[1] <= TSF_HIGH_GRAD_TOL, f"{worst[0]}: rel err {worst[1]:.3e} > {TSF_HIGH_GRAD_TOL:.1e}"


def _state(*models):
    return [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in models]


def test_a_recorded_plan_replays_at_the_tier_current_at_replay():
    """The recorded thunk calls the library's own entry point, which reads the tier when it dispatches: an eager and two planned steps (one
    recording, one replayed) at highest; a replayed step at high differs from highest and equals an eager high step; back at highest the replayed step
    is the eager highest step bit for bit (deterministic mode)."""
    prev_plans, prev_det = plans.ENABLED, L.set_deterministic(True)
    try:
        plans.ENABLED = True
        cfg, ef, tsf = harness.build_models(8, seed=4, device="cuda")
        opt = harness.make_optimizer(cfg, ef, tsf)
        batches = [harness.device_batch(2, 8, 2, seed=i, device="cuda") for i in range(4)]
        torch.manual_seed(5)

        def step(batch):
            y = harness.forward(ef, tsf, batch)
            loss = optim.bce_with_logits(y, batch["labels"], None)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            return y.detach().clone(), _state(ef, tsf)

        step(batches[0])                                  # eager
        recorded = plans.STATS["recorded"]
        step(batches[1])                                  # recorded
        assert plans.STATS["recorded"] == recorded + 2
        replayed = plans.STATS["replayed"]
        step(batches[2])                                  # replayed: two planned steps at highest before the tier changes
        assert plans.STATS["replayed"] == replayed + 4
        snap, rng = _state(ef, tsf), torch.cuda.get_rng_state()

        def from_snapshot(tier, planned):
            ef.load_state_dict(snap[0]), tsf.load_state_dict(snap[1])
            torch.cuda.set_rng_state(rng)
            plans.ENABLED = planned
            replayed = plans.STATS["replayed"]
            with mintime_amd.matmul_precision(tier):
                out = step(batches[3])
            assert plans.STATS["replayed"] == replayed + (4 if planned else 0), "the step must be a replay of the recorded plans"
            return out

        y_high_plan, _ = from_snapshot("high", True)
        y_top_plan, s_top_plan = from_snapshot("highest", True)
        y_high_eager, _ = from_snapshot("high", False)
        y_top_eager, s_top_eager = from_snapshot("highest", False)
    finally:
        plans.ENABLED = prev_plans
        L.set_deterministic(prev_det)
    assert not torch.equal(y_high_plan, y_top_plan), "the replayed step ignored the tier"
    assert_close(y_high_plan, y_high_eager, TOL, "replayed high step vs eager high step")
    assert torch.equal(y_top_plan, y_top_eager)
    diff = [k for s_p, s_e in zip(s_top_plan, s_top_eager) for k in s_e if not torch.equal(s_e[k], s_p[k])]
    assert not diff, f"{len(diff)} state tensors differ between the replayed and the eager highest step, e.g. {diff[:5]}"


def test_efficientnet_train_step_at_high():
    """EfficientNet-B0 train forward + backward at 16 crops (the late stages' 1x1 convolutions run on the plane loop): features at
    REL_TOL, every parameter gradient at EF_HIGH_GRAD_TOL, both against the fp64 oracle."""
    from mintime_amd import effnet_engine
    n, seed = 16, 5
    model = EfficientNet.from_name("efficientnet-b0", drop_connect_rate=0.0)
    sd = synth.effnet_b0_state(seed)
    model.load_state_dict(sd, strict=True)
    model.train(True)
    model = model.cuda()
    scope = effnet_engine.planes_scope(model, n)
    if not any(scope[0] + scope[1] + [scope[2]]):
        pytest.skip("the plane path is off (MT_GEMM_SPLIT=0)")
    x = synth.clip_inputs(1, n, 1, seed)["videos"].reshape(n, 224, 224, 3).permute(0, 3, 1, 2)
    gw = torch.randn(n, 1280, 7, 7, generator=torch.Generator().manual_seed(7)) * 0.1
    with mintime_amd.matmul_precision("high"):
        f = model(x.cuda())
        (f * gw.cuda()).sum().backward()
        torch.cuda.synchronize()
    osd = {k: (v.double().requires_grad_("running_" not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    fo = O.effnet_b0_forward(osd, x.double(), training=True)
    (fo * gw.double()).sum().backward()
    assert_close(f, fo, REL_TOL, "features at high vs oracle")
    named = dict(model.named_parameters())
    errs = []
    for k, p in named.items():
        if k.startswith("_fc"):
            continue
        ref = osd[k].grad
        wn = float(named[k.replace(".bias", ".weight")].grad.norm()) if k.endswith("_bn2.bias") else 0.0
        if k.endswith("_bn2.bias") and float(ref.norm()) < 1e-3 * wn:       # analytically zero in train mode (tests/test_gpu_effnet.py)
            assert float(p.grad.norm()) < 1e-3 * wn, k
            continue
        errs.append((k, rel_err(p.grad, ref)))
    worst = max(errs, key=lambda t: t[1])
    print(f"[precision] EfficientNet-B0 at high, 16 crops: features rel err {rel_err(f, fo):.3e}, worst gradient rel err "
          f"{worst[1]:.3e} ({worst[0]}) of {len(errs)}")
    assert EF_HIGH_GRAD_TOL <= REL_TOL
    assert worst[1] <= EF_HIGH_GRAD_TOL, f"grad {worst[0]}: rel err {worst[1]:.3e} > {EF_HIGH_GRAD_TOL:.1e}"
