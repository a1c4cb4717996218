"""CPU-only: tests/streaming_ops_ref.py against torch autograd of the composed fp64 MBConv block (expand conv -> BatchNorm -> swish ->
BatchNorm -> swish -> squeeze-excite gate -> project conv -> BatchNorm), its *_supported restatements against the library, and, by
arithmetic on the launch geometry, that every entry of the case tables reaches the branch it exists for (at 256 CUs, the MI355X)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as Fn

from mintime_amd import lib

from . import streaming_ops_ref as R
from .util import rel_err

TOL = 1e-12      # fp64 sums of a few hundred O(1) terms in two orders
CUS = 256
F64 = torch.float64


def _bn(z, gamma, beta, eps=1e-3):
    mean, var = z.mean(0), z.var(0, unbiased=False)
    istd = (var + eps).rsqrt()
    return (z - mean) * istd * gamma + beta, mean, istd


def _bn_bwd_coefficients(s1, s2, n, gamma, mean, istd):
    """dz = ka du + kb z + kc of a training-mode BatchNorm from s1 = sum du, s2 = sum du xhat."""
    return torch.stack([gamma * istd, -gamma * istd * istd * s2 / n, -gamma * istd * s1 / n + gamma * istd * istd * s2 * mean / n])


def test_references_are_the_autograd_of_the_composed_block():
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=F64) + 0.5
    n_img, hw, Cin, C, Co = 4, 5, 8, 32, 12
    rows = n_img * hw
    x, We, Wp = rn(rows, Cin).requires_grad_(), rn(C, Cin).requires_grad_(), rn(Co, C).requires_grad_()
    g0, b0, g1, b1, g2, b2 = ru(C), rn(C), ru(C), rn(C), ru(Co), rn(Co)
    dws, M, probe, res = ru(C), rn(C, C) * 0.3, rn(rows, Co), rn(rows, Cin)

    z_e = Fn.linear(x, We)
    u0, m0, i0 = _bn(z_e, g0, b0)
    zd = R.swish(u0) * dws                                   # a per-channel stand-in for the depthwise conv
    u, m1, i1 = _bn(zd, g1, b1)
    act = R.swish(u)
    pooled = act.reshape(n_img, hw, C).mean(1)
    gate = torch.sigmoid(pooled @ M)
    a = act * R.per_row(gate, hw, rows)
    z_p = Fn.linear(a, Wp)
    y, m2, i2 = _bn(z_p, g2, b2)
    loss = (y * probe).sum() + (x * res).sum()
    d = dict(zip("x We Wp a gate pooled u zd u0".split(), torch.autograd.grad(loss, (x, We, Wp, a, gate, pooled, u, zd, u0))))
    D = lambda t: t.detach()
    x_, We_, Wp_, zd_, z_p_, z_e_, gate_ = D(x), D(We), D(Wp), D(zd), D(z_p), D(z_e), D(gate)
    sc1, sh1 = g1 * D(i1), b1 - D(m1) * g1 * D(i1)

    # forward: expand conv (plain), project conv (gate mode) and the sums of its output; a pitched weight in both orientations
    wbuf = torch.full((C, Cin + 3), float("nan"), dtype=F64)
    wbuf[:, :Cin] = We_
    assert rel_err(R.conv1x1_rows(x_, wbuf, 0, C)[0], z_e_) <= TOL
    wtb = torch.full((Cin, C + 5), float("nan"), dtype=F64)
    wtb[:, :C] = We_.t()
    assert rel_err(R.conv1x1_rows(x_, wtb, 1, C)[0], z_e_) <= TOL
    out, s, q = R.conv1x1_rows(zd_, Wp_, 0, Co, 1, None, sc1, sh1, gate_, hw)
    assert rel_err(out, z_p_) <= TOL and rel_err(s, z_p_.sum(0)) <= TOL and rel_err(q, (z_p_ * z_p_).sum(0)) <= TOL

    # project conv backwards: bn2, weight gradient (gated), data gradient (BN-backward mode, the forward weight used transposed)
    xhat2 = (z_p_ - D(m2)) * D(i2)
    kp = _bn_bwd_coefficients(probe.sum(0), (probe * xhat2).sum(0), rows, g2, D(m2), D(i2))
    assert rel_err(R.conv1x1_wgrad(probe, z_p_, kp, zd_, sc1, sh1, gate_, hw, 7.0), d["Wp"] + 7.0) <= TOL
    da = R.conv1x1_rows(probe, Wp_, 1, C, 2, z_p_, kp[0], kp[1], kp[2])[0]
    assert rel_err(da, d["a"]) <= TOL
    # squeeze-excite stage: d gate, then du_d and the sums that give bn1's backward
    assert rel_err(R.se_stage(probe, z_p_, kp, Wp_, zd_, sc1, sh1, 0, hw, dgate0=7.0)[0], d["gate"] + 7.0) <= TOL
    mi1 = torch.stack([D(m1), D(i1)])
    dud, s1, s2 = R.se_stage(probe, z_p_, kp, Wp_, zd_, sc1, sh1, 1, hw, gate_, d["pooled"], mi1)
    assert rel_err(dud, d["u"]) <= TOL
    k1 = _bn_bwd_coefficients(s1, s2, rows, g1, D(m1), D(i1))
    assert rel_err(k1[0] * dud + k1[1] * zd_ + k1[2], d["zd"]) <= TOL
    # expand conv backwards: bn0, then both gradients, fused and as the two single kernels
    du0 = d["u0"]
    xhat0 = (z_e_ - D(m0)) * D(i0)
    k0 = _bn_bwd_coefficients(du0.sum(0), (du0 * xhat0).sum(0), rows, g0, D(m0), D(i0))
    dx, dw = R.conv1x1_bwd_fused(du0, k0, x_, We_, res, 7.0)
    assert rel_err(dx, d["x"]) <= TOL and rel_err(dw, d["We"] + 7.0) <= TOL
    assert rel_err(R.conv1x1_bwd_fused(du0, k0, x_, We_)[0], d["x"] - res) <= TOL
    assert rel_err(R.conv1x1_wgrad(du0, z_e_, k0, x_), d["We"]) <= TOL
    assert rel_err(R.conv1x1_rows(du0, We_, 1, Cin, 2, z_e_, k0[0], k0[1], k0[2], res=res)[0], d["x"]) <= TOL


# ---- the *_supported restatements against the library ------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    h = ctypes.CDLL(lib.LIB_PATH)
    for name, n in (("mt_conv1x1_rows_supported", 3), ("mt_conv1x1_wgrad_supported", 2), ("mt_conv1x1_wgrad_wide_supported", 2),
                    ("mt_conv1x1_bwd_fused_supported", 2), ("mt_se_stage_fused_supported", 3)):
        getattr(h, name).argtypes = [ctypes.c_int] * n
        getattr(h, name).restype = ctypes.c_int
    return h


def test_supported_predicates_over_a_grid(handle):
    side = list(range(-1, 353))
    bad = []
    for a in side:
        for b in side:
            if handle.mt_conv1x1_wgrad_supported(a, b) != int(R.wgrad_supported(a, b)):
                bad.append(("wgrad", a, b))
            if handle.mt_conv1x1_bwd_fused_supported(a, b) != int(R.fused_supported(a, b)):
                bad.append(("fused", a, b))
            for amode in (0, 1, 2):
                if handle.mt_conv1x1_rows_supported(a, b, amode) != int(R.rows_supported(a, b, amode)):
                    bad.append(("rows", a, b, amode))
    for co in side:                                           # the wide kernel's Cin reaches 2048
        for ci in list(range(180, 353)) + list(range(2040, 2060)) + [480, 672, 1152, 1153, 1156]:
            if handle.mt_conv1x1_wgrad_wide_supported(co, ci) != int(R.wide_supported(co, ci)):
                bad.append(("wide", co, ci))
    for co in range(-1, 38):
        for c in list(range(28, 36)) + list(range(92, 100)) + list(range(140, 148)) + [0, 64, 128, 240, 352]:
            for hw in range(-1, 258):
                if handle.mt_se_stage_fused_supported(co, c, hw) != int(R.se_supported(co, c, hw)):
                    bad.append(("se", co, c, hw))
    assert not bad, bad[:20]
    assert handle.mt_se_stage_fused_supported(24, 96, 3136) == 1 and handle.mt_conv1x1_rows_supported(24, 144, 1) == 0


# ---- every table entry reaches what it is in the table for ------------------------------------------------------------------------------


def test_rows_table_reach():
    T = R.ROWS_CASES
    assert all(R.rows_built(c[0], c[1]) for c in T)
    assert {(R.tiles(c[0]), R.tiles(c[1])) for c in T} == R.ROWS_INSTANCES
    assert {c[0] for c in T} >= {4, 16, 24, 28, 32, 72, 96} and {c[1] for c in T} >= {1, 16, 96, 129, 144}
    assert any(c[1] % 4 for c in T) and {c[2] for c in T} == {0, 1, 2}
    assert {c[3] for c in T} >= {1, 31, 127, 128, 129}
    assert {(c[5] > 0, c[6]) for c in T} == {(False, 0), (True, 0), (False, 1), (True, 1)}      # pitch x orientation
    assert {c[7] for c in T} == {False, True}
    forms = {f for c in T for f in c[8]}
    assert forms >= {0, 1, 8, 32, -8, -32}
    gated = [c for c in T if c[2] == 1]
    assert sorted(c[4] for c in gated) == [1, 7, 49, 128, R.BIG]
    for Cin, Cout, amode, rows, hw, *_ in gated:
        walk = R.rows_walk(rows)
        per_chunk = R.images_in_chunk(walk, hw, 0)
        assert {1: per_chunk == 128, 7: per_chunk >= 18, 49: per_chunk >= 3, 128: per_chunk == 1 and walk.nchunks > 2,
                R.BIG: per_chunk == 1 and hw > rows}[hw]
    big = [c for c in T if c[3] > 512 * 128]
    assert len(big) == 1
    walk = R.rows_walk(big[0][3])
    assert walk.grid == 512 and sorted(set(walk.counts())) == [1, 2] and big[0][3] % 128 not in (0,)
    assert all(abs(f) < 512 for f in big[0][8] if f) and any(f < 0 for f in big[0][8])          # blockIdx % slots wraps, limbs too
    assert bool(R.rows_walk(big[0][3]).later_rows().any())


def test_wgrad_table_reach():
    T = R.WGRAD_CASES
    assert all(R.wgrad_supported(c[0], c[1]) and c[0] % 32 and c[1] % 32 for c in T)
    small = T[:18]
    assert {(R.tiles(c[0]), R.tiles(c[1])) for c in small} == set(R.WGRAD_INSTANCES)
    assert any(c[3] == 0 for c in T) and any(c[3] for c in T)
    kinds, hws = set(), set()
    for Cout, Cin, rows, hw in small:
        Rr = R.wgrad_walk(rows, Cout, Cin).R
        kinds.add("1" if rows == 1 else "R-1" if rows == Rr - 1 else "R+1" if rows == Rr + 1 else "more")
        if hw:
            hws.add("R" if hw == Rr else hw)
    assert kinds == {"1", "R-1", "R+1", "more"} and hws == {1, 7, 49, "R", R.BIG}
    reached = set()
    for Cout, Cin, rows, hw in T[18:]:
        walk = R.wgrad_walk(rows, Cout, Cin)
        bpc = R.WGRAD_INSTANCES[(R.tiles(Cout), R.tiles(Cin))][3]
        assert rows > 256 * bpc * walk.R and rows % walk.R and sorted(set(walk.counts())) == [1, 2]
        reached.add((walk.R, R.wgrad_row_groups(Cout, Cin)))
        if hw:
            assert R.images_in_chunk(walk, hw, 1) >= 1
    assert reached == {(128, 4), (64, 4), (32, 4), (32, 2), (32, 1)}
    assert any(R.WGRAD_INSTANCES[(R.tiles(c[0]), R.tiles(c[1]))][3] == 1 for c in T[18:])        # the one-block-per-CU cap
    assert any(hw == R.wgrad_walk(rows, co, ci).R for co, ci, rows, hw in T[18:])                # hw = chunk height across chunks
    assert any(not R.WGRAD_INSTANCES[(R.tiles(c[0]), R.tiles(c[1]))][4] for c in T)              # coefficients from LDS


def test_wide_table_reach():
    T = R.wide_cases(CUS)
    assert all(R.wide_supported(c[0], c[1]) for c in T)
    assert {R.tiles(c[0]) for c in T} == set(R.WIDE_TILES)
    assert {c[0] for c in T} == {68, 80, 112, 100, 192, 164, 320, 292}
    assert {c[1] for c in T} == {224, 240, 672, 1152, 2048} and {c[3] for c in T} == {32, 49, 196}
    assert 672 - 128 * (R.cdiv(672, 128) - 1) == 32 and R.cdiv(1152, 128) == 9 and R.cdiv(2048, 128) == 16 and 240 % 128
    seen = set()
    for Cout, Cin, rows, hw, why in T:
        nslab, nsplit, cps, nchunks = R.wide_plan(rows, Cin, CUS)
        counts = R.wide_walk(rows, Cin, CUS).counts()
        if why == "idle":
            assert nchunks < nsplit and counts.count(0) >= 1 and cps == 1
        else:
            assert cps == int(why[3:]) and rows % 32
            assert (counts.count(0) >= 1) if cps == 1 else (min(c for c in counts if c) < cps)      # idle splits / a shorter last range
        seen.add(cps)
        if R.tiles(Cout) == 10 and cps >= 3:
            seen.add("single set, several chunks")
        if hw == 32:
            assert all((c * 32) % hw == 0 for c in range(nchunks))         # every chunk starts an image: the two-image rule at its edge
        else:
            assert any(R.images_in_chunk(R.wide_walk(rows, Cin, CUS), hw, c) == 2 for c in range(nchunks)) or rows <= hw
    assert seen >= {1, 2, 3, 4, 5, "single set, several chunks"}


def test_fused_table_reach():
    T = R.fused_cases(CUS)
    assert all(R.fused_supported(c[0], c[1]) for c in T)
    assert {(c[0], c[1]) for c in T} >= {(96, 4), (96, 16), (96, 20), (96, 24), (96, 32), (144, 8), (144, 16), (144, 24), (144, 32)}
    assert {R.fused_instance(c[0], c[1]) for c in T} == {(3, True), (3, False), (5, False)}
    assert {c[2] for c in T} >= {1, 64} and {c[3] for c in T} == {False, True}
    mixes = {}
    for Cout, Cin, rows, res in T:
        counts = sorted(set(R.fused_walk(rows, CUS).counts()))
        if len(counts) == 2:
            mixes.setdefault(R.fused_instance(Cout, Cin), set()).add((tuple(counts), rows % 64))
    for inst, m in mixes.items():
        assert {c for c, _ in m} == {(1, 2), (4, 5)}, inst          # 4 and 5: both in-loop drains and both after the loop
    assert len(mixes) == 3
    assert {t for m in mixes.values() for _, t in m} == {1, 63}
    assert max(c[2] * c[0] for c in T) * 4 < 48 << 20


def test_se_table_reach():
    T = R.SE_CASES
    assert all(R.se_supported(c[0], c[1], c[2]) for c in T)
    assert {c[1] for c in T} == {32, 96, 144} and {c[0] for c in T} == {4, 16, 24, 32}
    assert (24, 144, 64, 2) in {c[:4] for c in T}
    forms = {f for c in T for f in c[4]}
    assert any(f > 0 for f in forms) and any(f < 0 for f in forms)
    three, straddle = False, False
    for Co, C, hw, n_img, _ in T:
        walk = R.se_walk(n_img * hw)
        for b in range(walk.grid):
            imgs = [c * 64 // hw for c in walk.chunks_of(b)]
            if len(set(imgs)) >= 3:
                three = three or (hw == 64 and n_img > 1024)
            if hw == 192 and len(imgs) == 2 and imgs[0] != imgs[1] and walk.chunks_of(b)[0] * 64 % hw:
                straddle = True          # starts inside one image, ends in the next: the in-loop flush with a part-image sum
    assert three and straddle
    assert max(c[2] * c[3] * c[1] for c in T) * 4 < 48 << 20
