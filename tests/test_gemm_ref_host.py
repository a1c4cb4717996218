"""CPU-only checks of what the GEMM parity tests stand on (tests/gemm_ref.py, tests/gemm_cases.py): the fused references against torch
autograd in fp64, the section-wise comparison against single planted errors that the whole-tensor metric misses, and the conditioning
of every summed output of every GPU case."""
import pytest
import torch

from . import gemm_cases as G
from . import gemm_ref as R
from .util import rel_err

F64 = torch.float64
N_IMG, HW, CEXP, COUT = 3, 5, 12, 8
M = N_IMG * HW


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


@pytest.fixture(scope="module")
def mbconv_tail():
    """a = swish(z_d sc + sh) gate[img], z_p = a Wp^T; dz_p = ka du + kb z_p + kc is the cotangent of z_p, e_dpool that of the pooled
    activation mean_hw swish(u).  Autograd's gradients with respect to gate, u = z_d sc + sh and Wp."""
    g = torch.Generator().manual_seed(5)
    t = dict(z_d=_rn(g, M, CEXP), sc=torch.rand(CEXP, generator=g, dtype=F64) + 0.5, sh=_rn(g, CEXP) * 0.3,
             gate=torch.sigmoid(_rn(g, N_IMG, CEXP)), Wp=_rn(g, COUT, CEXP) * 0.3, du=_rn(g, M, COUT),
             ka=torch.rand(COUT, generator=g, dtype=F64) + 0.5, kb=_rn(g, COUT) * 0.1, kc=_rn(g, COUT) * 0.2,
             e_dpool=_rn(g, N_IMG, CEXP), mi=torch.cat((_rn(g, CEXP) * 0.1, torch.rand(CEXP, generator=g, dtype=F64) + 0.5)))
    u = (t["z_d"] * t["sc"] + t["sh"]).requires_grad_(True)
    gate, Wp = t["gate"].clone().requires_grad_(True), t["Wp"].clone().requires_grad_(True)
    act = R.swish(u)
    z_p = (act * gate.repeat_interleave(HW, 0)) @ Wp.T
    t["z_p"] = z_p.detach()
    dz_p = t["ka"] * t["du"] + t["kb"] * t["z_p"] + t["kc"]
    pooled = act.reshape(N_IMG, HW, CEXP).mean(1)
    # the gate receives the project path only; u receives it through the fixed gate plus the pooled path
    t["d_gate"], t["d_Wp"] = torch.autograd.grad((z_p * dz_p).sum(), (gate, Wp), retain_graph=True)
    t["d_u"], = torch.autograd.grad((z_p * dz_p).sum() + (pooled * t["e_dpool"]).sum(), u)
    return t


def _se_call(t, epilogue, Cout):
    epi = (t["sc"], t["sh"], t["gate"], t["e_dpool"], t["mi"], HW)
    return R.gemm(R.OP_NN, t["du"], t["Wp"], Cout, M, CEXP, COUT, COUT, CEXP, CEXP, prologue=R.PRO_BN_BWD, epilogue=epilogue, scale=t["ka"],
                  shift=t["kb"], gate=t["kc"], A2=t["z_p"], C2=t["z_d"], ldc2=CEXP, epi=epi)


def test_se_red_is_autograds_gate_gradient(mbconv_tail):
    t = mbconv_tail
    out = _se_call(t, R.EPI_SE_RED, torch.zeros(N_IMG, CEXP, dtype=F64))
    assert rel_err(out["C"], t["d_gate"]) < 1e-13


def test_act_bwd_is_autograds_preactivation_gradient_and_its_sums(mbconv_tail):
    t = mbconv_tail
    out = _se_call(t, R.EPI_ACT_BWD, torch.zeros(M, CEXP, dtype=F64))
    assert rel_err(out["C"], t["d_u"]) < 1e-13
    xhat = (t["z_d"] - t["mi"][:CEXP]) * t["mi"][CEXP:]
    assert rel_err(out["stats"][0], t["d_u"].sum(0)) < 1e-13
    assert rel_err(out["stats"][1], (t["d_u"] * xhat).sum(0)) < 1e-13


def test_b_prologue_weight_gradient_is_autograds(mbconv_tail):
    t = mbconv_tail
    out = R.gemm(R.OP_TN, t["du"], t["z_d"], torch.zeros(COUT, CEXP, dtype=F64), COUT, CEXP, M, COUT, CEXP, CEXP, prologue=R.PRO_BN_BWD,
                 epilogue=R.EPI_ATOMIC, scale=t["ka"], shift=t["kb"], gate=t["kc"], A2=t["z_p"], b_prologue=R.BPRO_BN_SWISH_GATE,
                 b_scale=t["sc"], b_shift=t["sh"], b_gate=t["gate"], b_hw=HW)
    assert rel_err(out["C"], t["d_Wp"]) < 1e-13


@pytest.mark.parametrize("form", ["NN", "NT"])
def test_geglu_bwd_is_autograd_of_a_gelu_g(form):
    g = torch.Generator().manual_seed(6)
    rows, D, nh = 7, 8, 12
    dy, W2, u = _rn(g, rows, D), _rn(g, D, nh) * 0.3, _rn(g, rows, 2 * nh).requires_grad_(True)
    a, gg = u[:, :nh], u[:, nh:]
    want, = torch.autograd.grad((a * torch.nn.functional.gelu(gg) * (dy @ W2)).sum(), u)
    u_il = torch.stack((a.detach(), gg.detach()), dim=-1).reshape(rows, 2 * nh).contiguous()
    cs0 = torch.full((2 * nh,), 3.0, dtype=F64)
    C = torch.zeros(rows, 2 * nh, dtype=F64)
    kw = dict(epilogue=R.EPI_GEGLU_BWD, C2=u_il, ldc2=2 * nh, n_half=nh, col_sum=cs0)
    if form == "NN":
        out = R.gemm(R.OP_NN, dy, W2, C, rows, nh, D, D, nh, 2 * nh, **kw)
    else:
        out = R.gemm(R.OP_NT, dy, W2.T.contiguous(), C, rows, nh, D, D, D, 2 * nh, **kw)
    assert rel_err(out["C"], want) < 1e-13
    assert rel_err(out["col_sum"], 3.0 + want.sum(0)) < 1e-13


def test_geglu_forward_and_row_maps():
    """GEGLU against torch's gelu with the pre-activations interleaved; a_map / b_map / c_map against explicit indexing."""
    g = torch.Generator().manual_seed(7)
    rows, D, nh = 6, 8, 4
    x, W, b = _rn(g, rows, D), _rn(g, 2 * nh, D), _rn(g, 2 * nh)
    out = R.gemm(R.OP_NT, x, W, torch.zeros(rows, nh, dtype=F64), rows, 2 * nh, D, D, D, nh, epilogue=R.EPI_GEGLU, bias=b,
                 C2=torch.zeros(rows, 2 * nh, dtype=F64), ldc2=2 * nh, n_half=nh)
    u = x @ W.T + b
    assert rel_err(out["C"], u[:, :nh] * torch.nn.functional.gelu(u[:, nh:])) < 1e-13
    assert torch.equal(out["C2"][:, 0::2], u[:, :nh]) and torch.equal(out["C2"][:, 1::2], u[:, nh:])
    # rows 0..5 of a [2 x 3]-grouped operand live at memory rows 1, 2, 3, 5, 6, 7 (gin 3, gout 4, off 1)
    rm, idx = (3, 4, 1), torch.tensor([1, 2, 3, 5, 6, 7])
    Aw, Bw = _rn(g, 8, D), _rn(g, 8, nh)
    C0 = _rn(g, 8, nh)
    out = R.gemm(R.OP_TN, Aw, Bw, C0, D, nh, 6, D, nh, nh, epilogue=R.EPI_ATOMIC, a_map=rm, b_map=rm)
    assert rel_err(out["C"], C0[:D] + Aw[idx].T @ Bw[idx]) < 1e-13
    out = R.gemm(R.OP_NN, x, Bw, C0, rows, nh, D, D, nh, nh, epilogue=R.EPI_ACCUM, c_map=rm)
    assert rel_err(out["C"], C0[idx] + x @ Bw) < 1e-13


# ---- the im2col forms against F.conv2d and its autograd ----------------------------------------------------------------------------

# (n, H, W, C, Cout, k, stride, pad, extra rows, extra columns of output beyond the floor formula, affine, relu, uint8)
CONV_GEOS = [
    (2, 6, 6, 4, 5, 3, 1, 1, 0, 0, True, True, False),
    (2, 7, 10, 4, 3, 3, 1, 0, 0, 0, False, False, False),      # H != W, valid
    (3, 10, 14, 3, 6, 3, 2, 0, 1, 1, False, False, True),      # the SAME overhang of an even size: Ho = ceil(H / 2) at pad 0
    (2, 9, 13, 3, 6, 3, 2, 1, 0, 0, False, False, True),       # odd sizes, leading pad 1
    (2, 9, 13, 3, 6, 3, 2, 0, 0, 0, True, False, False),
    (2, 13, 18, 4, 7, 5, 2, 2, 0, 0, True, False, False),
    (2, 4, 6, 4, 3, 3, 1, 3, 0, 0, True, True, False),         # padding >= k
    (3, 9, 12, 8, 5, 1, 2, 0, 0, 0, True, True, False),        # strided 1 x 1
    (2, 12, 15, 4, 3, 7, 2, 3, 0, 0, True, True, False),
    (1, 5, 8, 2, 3, 2, 3, 1, 1, 0, True, True, False),         # even kernel, stride 3, overhang on the rows only
    (2, 8, 5, 5, 4, 3, 1, 2, 0, 0, False, True, True),         # "full" padding p = k - 1, C % 4 != 0
]


def _conv_problem(geo, seed):
    """Image, affine, weights (torch layout and packed [(kh, kw, ci)] with noise in the padding columns) and the fp64 activation
    a = act(affine(x)) zero-padded so that F.conv2d at padding 0 gives exactly Ho x Wo windows."""
    import torch.nn.functional as F
    n, H, W, C, Cout, k, s, p, eh, ew, aff, relu, u8 = geo
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * p - k) // s + 1 + eh, (W + 2 * p - k) // s + 1 + ew
    x = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8) if u8 else _rn(g, n, H, W, C)
    sc, sh = (torch.rand(C, generator=g, dtype=F64) + 0.5, _rn(g, C)) if aff else (None, None)
    w = _rn(g, Cout, C, k, k).requires_grad_(True)
    kk = k * k * C
    K = (kk + 3) // 4 * 4
    wp = _rn(g, Cout, K)
    wp[:, :kk] = w.detach().permute(0, 2, 3, 1).reshape(Cout, kk)
    a = x.to(F64)
    if aff:
        a = a * sc + sh
    if relu:
        a = a.clamp_min(0)
    a = a.permute(0, 3, 1, 2)
    pb, pr = max(0, (Ho - 1) * s + k - p - H), max(0, (Wo - 1) * s + k - p - W)
    a_pad = F.pad(a, (p, pr, p, pb))
    conv = (H, W, C, Ho, Wo, k, s, p, R.ACT_RELU if relu else R.ACT_NONE, int(u8))
    return dict(x=x, sc=sc, sh=sh, w=w, wp=wp, a_pad=a_pad, conv=conv, M=n * Ho * Wo, K=K, kk=kk, Cout=Cout, Ho=Ho, Wo=Wo, s=s, g=g)


@pytest.mark.parametrize("geo", CONV_GEOS, ids=lambda g: "x".join(map(str, g[:10])))
def test_im2col_forward_is_conv2d(geo):
    import torch.nn.functional as F
    t = _conv_problem(geo, 21)
    out = R.gemm(R.OP_NT, t["x"].reshape(-1), t["wp"], None, t["M"], t["Cout"], t["K"], t["K"], t["K"], t["Cout"],
                 prologue=R.PRO_IM2COL, scale=t["sc"], shift=t["sh"], conv=t["conv"])
    want = F.conv2d(t["a_pad"], t["w"].detach(), None, t["s"])[:, :, :t["Ho"], :t["Wo"]]
    assert want.shape[2:] == (t["Ho"], t["Wo"])
    assert rel_err(out["C"], want.permute(0, 2, 3, 1).reshape(t["M"], t["Cout"])) < 1e-13
    a, _ = R.operands(R.OP_NT, t["x"].reshape(-1), t["wp"], t["M"], t["Cout"], t["K"], t["K"], t["K"], prologue=R.PRO_IM2COL,
                      scale=t["sc"], shift=t["sh"], conv=t["conv"])
    assert not a[:, t["kk"]:].any()                  # the padding columns of K are exactly zero, whatever the weights hold there


@pytest.mark.parametrize("geo", CONV_GEOS, ids=lambda g: "x".join(map(str, g[:10])))
def test_im2col_weight_gradient_is_autograds(geo):
    import torch.nn.functional as F
    t = _conv_problem(geo, 22)
    g, M, Cout, K, kk = t["g"], t["M"], t["Cout"], t["K"], t["kk"]
    du, z = _rn(g, M, Cout), _rn(g, M, Cout)
    ka, kb, kc = torch.rand(Cout, generator=g, dtype=F64) + 0.5, _rn(g, Cout) * 0.1, _rn(g, Cout) * 0.2
    C0 = _rn(g, Cout, K)
    out = R.gemm(R.OP_TN, du, t["x"].reshape(-1), C0, Cout, K, M, Cout, K, K, prologue=R.PRO_BN_BWD, epilogue=R.EPI_ATOMIC, scale=ka,
                 shift=kb, gate=kc, A2=z, b_prologue=R.BPRO_IM2COL, b_scale=t["sc"], b_shift=t["sh"], conv=t["conv"])
    dz = (ka * du + kb * z + kc).reshape(-1, t["Ho"], t["Wo"], Cout).permute(0, 3, 1, 2)
    y = F.conv2d(t["a_pad"], t["w"], None, t["s"])[:, :, :t["Ho"], :t["Wo"]]
    dw, = torch.autograd.grad(y, t["w"], dz)
    assert rel_err(out["C"][:, :kk], C0[:, :kk] + dw.permute(0, 2, 3, 1).reshape(Cout, kk)) < 1e-13
    assert torch.equal(out["C"][:, kk:], C0[:, kk:])  # the output's padding columns keep what they held, exactly


@pytest.mark.parametrize("shape", [(2, 7, 10, 4, 6, 3), (1, 9, 6, 8, 4, 5), (2, 5, 5, 4, 4, 1)], ids=str)
def test_im2col_full_correlation_is_autograds_data_gradient(shape):
    """The data gradient of a stride-1 valid convolution as the engines run it (Xception conv2): the im2col form over the OUTPUT
    gradient with pad = k - 1 and the weights transposed and flipped, wt[ci][(kh, kw, co)] = w[co, ci, k-1-kh, k-1-kw]."""
    import torch.nn.functional as F
    n, H, W, Cin, Cout, k = shape
    g = torch.Generator().manual_seed(23)
    x, w = _rn(g, n, Cin, H, W).requires_grad_(True), _rn(g, Cout, Cin, k, k)
    H2, W2 = H - k + 1, W - k + 1
    dy = _rn(g, n, H2, W2, Cout)
    want, = torch.autograd.grad(F.conv2d(x, w), x, dy.permute(0, 3, 1, 2))
    wt = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, k * k * Cout).contiguous()
    K = k * k * Cout
    out = R.gemm(R.OP_NT, dy.reshape(-1), wt, None, n * H * W, Cin, K, K, K, Cin, prologue=R.PRO_IM2COL,
                 conv=(H2, W2, Cout, H, W, k, 1, k - 1, R.ACT_NONE))
    assert rel_err(out["C"], want.permute(0, 2, 3, 1).reshape(n * H * W, Cin)) < 1e-13


# ---- the im2col cases can tell a wrong kernel from a right one ----------------------------------------------------------------------

def _wrong_im2col(wrong):
    """R.im2col with one planted mistake (None: none), written by flat addressing, not by indexing a 4-D image:
      a  the padding goes through the affine and the activation        b  leading pad off by one (p - 1)
      c  H and W swapped in the addressing                              d  the columns from k k C on decoded as (tap, channel) and gathered
      e  uint8 read as int8                                             f  the pixel cursor does not wrap at an image boundary: image
                                                                           n + 1 is read at the rows following image n's last window"""
    def f(x, conv, rows, cols, scale, shift, dt):
        H, W, C, Ho, Wo, k, s, p, act = conv[:9]
        n_img = (rows - 1) // (Ho * Wo) + 1
        flat = x.reshape(-1)[:n_img * H * W * C].to(dt)
        if wrong == "e" and len(conv) > 9 and conv[9]:
            flat = torch.where(flat >= 128, flat - 256, flat)
        if wrong == "b":
            p = p - 1
        aH, aW = (W, H) if wrong == "c" else (H, W)
        r = torch.arange(rows)
        ow = r % Wo
        if wrong == "f":
            n, oh, rows_in = torch.zeros_like(r), r // Wo, n_img * H
        else:
            n, oh, rows_in = r // (Ho * Wo), (r // Wo) % Ho, aH
        out = torch.zeros(rows, cols, dtype=dt)
        for tap in range((cols - 1) // C + 1 if wrong == "d" else k * k):
            kh, kw = tap // k, tap % k
            ih, iw = oh * s + kh - p, ow * s + kw - p
            ok = (ih >= 0) & (ih < rows_in) & (iw >= 0) & (iw < aW)
            idx = (((n * aH + ih) * aW + iw) * C).clamp(0, flat.numel() - C)
            v = flat[idx[:, None] + torch.arange(C)] * ok[:, None]
            live = torch.ones_like(ok) if wrong == "a" else ok
            if scale is not None:
                v = torch.where(live[:, None], v * scale.to(dt)[:C] + shift.to(dt)[:C], v)
            if act == R.ACT_RELU:
                v = v.clamp_min(0)
            width = min(C, cols - tap * C)
            out[:, tap * C:tap * C + width] = v[:, :width]
        return out
    return f


def _im2col_probe_cases():
    """One tile per input: the A-side cases of MT_FORCE_CFG 3 (64 x 64 sections) and the B-side cases with one K range."""
    return G.im2col_a_cases(3) + [c for c in G.im2col_b_cases() if c.split_k == 1]


def _eval64(case):
    b = G.inputs(case)
    v = b.views({k: t.double() for k, t in b.wide.items()})
    v["stats"] = None
    return b.call(R.gemm, v)


def _worst_over_gate(case, out, ref):
    """max over the sections of C (and of the two sums) of figure / gate."""
    bm, bn = case.tile
    worst = max(e for _, e in G.sections(out["C"], ref["C"], bm, bn)) / G.TOL[case.kind]
    if "stats" in ref:
        for i in range(2):
            worst = max(worst, max(e for _, e in G.sum_sections(out["stats"][i], ref["stats"][i], bn)) / G.TOL[case.prefix + "sums"])
    return worst


def test_planted_variant_without_a_mistake_is_the_reference(monkeypatch):
    monkeypatch.setattr(R, "im2col", _wrong_im2col(None))
    for c in _im2col_probe_cases():
        out, ref = _eval64(c), G.reference(c)
        for k in ref:
            assert torch.equal(out[k], ref[k]), (c.name, k)


@pytest.mark.parametrize("wrong", list("abcdef"))
def test_im2col_cases_separate_a_wrong_kernel(wrong, monkeypatch):
    """For each planted mistake at least one case in which the mistaken matrix, evaluated in fp64, lies more than 1000 gates from the
    reference in some section.  A property of the inputs and the reference; the library is not run.  What separates what (printed):
    the A-side and the B-side group are both required wherever the mistake can exist on that side."""
    refs = {c: G.reference(c) for c in _im2col_probe_cases()}
    monkeypatch.setattr(R, "im2col", _wrong_im2col(wrong))
    hit = {}
    for c, ref in refs.items():
        ratio = _worst_over_gate(c, _eval64(c), ref)
        if ratio > 1000:
            hit[c.name] = ratio
    for name, ratio in hit.items():
        print(f"SEPARATES {wrong} | {name} | {ratio:.3g} gates")
    a_side = [n for n in hit if "wgrad" not in n]
    b_side = [n for n in hit if "wgrad" in n]
    if wrong != "f":                                 # (f) is the B side's cursor
        assert a_side, f"no A-side case separates variant ({wrong})"
    if wrong != "d":                                 # (d) on the B side is the exact check of the output's padding columns
        assert b_side, f"no B-side case separates variant ({wrong})"


def test_split_3_starts_a_range_inside_an_image_row():
    """Every weight-gradient case at split_k 3: some K range begins in the middle of an image row (the pixel cursor starts from
    k_begin), by the library's own split_k_ranges.  Wo 16 cannot: every multiple of the 16-pixel k-step is the start of a row."""
    import ctypes
    import os
    from mintime_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    h = ctypes.CDLL(lib.LIB_PATH)
    h.mt_debug_split_k.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)]
    h.mt_debug_split_k.restype = None
    seen = 0
    for c in G.im2col_b_cases():
        if c.split_k != 3:
            continue
        Ho, Wo = c.conv[3:5]
        assert c.K == G.IM2COL_B_IMAGES * Ho * Wo
        bm, bn = c.tile
        tiles = ((c.M + bm - 1) // bm) * ((c.N + bn - 1) // bn)
        out = (ctypes.c_int * 4)()
        h.mt_debug_split_k(c.K, tiles, 3, 2048, 16, 0, out)
        k_chunk, ranges = out[0], out[1]
        assert ranges == 3, c.name
        mid_row = any((i * k_chunk) % Wo for i in range(1, ranges))
        assert mid_row == (Wo != 16), (c.name, k_chunk)
        # an image boundary inside a 16-pixel k-step, wherever Ho Wo is no multiple of 16
        assert ((Ho * Wo) % 16 != 0) == (Wo != 16), c.name
        seen += 1
    assert seen == len(G.IM2COL_B) + 3


def test_weight_gradient_cases_name_the_tile_the_library_picks(monkeypatch):
    """The tile column of IM2COL_B, by which the comparison is cut into sections, is the library's own choice for that call (gemm.hip:
    pick_cfg and the one-tile configuration), and both sides of the one-tile condition are in the list."""
    import ctypes
    import os
    from mintime_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    monkeypatch.delenv("MT_FORCE_CFG", raising=False)
    h = ctypes.CDLL(lib.LIB_PATH)
    h.mt_debug_gemm_tile.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)]
    h.mt_debug_gemm_tile.restype = None
    tiles = set()
    for c in G.im2col_b_cases():
        out = (ctypes.c_int * 2)()
        h.mt_debug_gemm_tile(c.op, c.M, c.N, c.pro, c.bpro, c.epi, out)
        assert tuple(out) == c.tile, c.name
        tiles.add(c.tile)
    assert tiles == {(128, 128), (128, 64), (256, 32), (64, 288)}


# ---- the sections see what the whole-tensor metric misses --------------------------------------------------------------------------

BM = BN = 64
ROWS, COLS, IMG = 3 * 64 + 4, 2 * 64 + 4, 49            # 4 row tiles (the last of 4 rows), 3 column tiles (the last of 4), 4 images
GATE = max(v for k, v in G.TOL.items() if not k.startswith("high."))


def _over(figs):
    return {name for name, e in figs if e > GATE}


def _planted(scale_rows=None, scale_cols=None):
    ref = torch.randn(ROWS, COLS, generator=torch.Generator().manual_seed(8), dtype=F64)
    if scale_rows is not None:
        ref[scale_rows] *= 1e-3
    if scale_cols is not None:
        ref[:, scale_cols] *= 1e-3
    return ref


def test_sections_see_one_element_of_the_last_column_tile():
    ref = _planted(scale_cols=slice(128, COLS))
    ref[100, 130] = 2e-3
    got = ref.clone()
    got[100, 130] *= 1 + 1e-3
    assert _over(G.sections(got, ref, BM, BN)) == {"last column tile"}
    assert rel_err(got, ref) < 2e-5


def test_sections_see_one_element_of_the_last_row_tile():
    ref = _planted(scale_rows=slice(192, ROWS))
    ref[194, 70] = 2e-3
    got = ref.clone()
    got[194, 70] *= 1 + 1e-3
    assert _over(G.sections(got, ref, BM, BN)) == {"last row tile"}
    assert rel_err(got, ref) < 2e-5


def test_sections_see_the_first_row_of_an_interior_image():
    ref = _planted()
    ref[IMG:2 * IMG] *= 1e-5                       # image 1 is small: its rows hide in every tile section
    got = ref.clone()
    got[IMG] *= 1 + 1e-3
    assert _over(G.sections(got, ref, BM, BN, hw=IMG)) == {"worst image"}
    assert rel_err(got, ref) < 2e-5


def test_sections_see_one_entry_of_col_sum():
    ref = torch.randn(COLS, generator=torch.Generator().manual_seed(9), dtype=F64) + 3.0
    ref[128:] *= 1e-3
    got = ref.clone()
    got[130] *= 1 + 1e-3
    assert _over(G.sum_sections(got, ref, BN)) == {"last column tile"}
    assert rel_err(got, ref) < 2e-5


def test_sections_report_a_nan_left_behind():
    ref = _planted()
    got = ref.clone()
    got[70, 70] = float("nan")
    assert _over(G.sections(got, ref, BM, BN)) == {"interior"}


def test_l2_blocked_cases_have_the_intended_geometry():
    """tests/gemm_cases.py l2_cases: 34 x 3 tiles of 64 x 64 on a grid padded to 8 x 5 rows of tiles; group_n 2 at K 4092 (the last
    group one tile wide), 1 at K 4100 -- from the library's own tile_grid (csrc/gemm_geometry.hpp)."""
    import ctypes
    import os
    from mintime_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    h = ctypes.CDLL(lib.LIB_PATH)
    h.mt_debug_tile_grid.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
    h.mt_debug_tile_grid.restype = None
    want = {4092: (34, 3, 120, 2), 4100: (34, 3, 120, 1)}
    for c in G.l2_cases():
        out = (ctypes.c_int * 4)()
        h.mt_debug_tile_grid(c.M, c.N, *c.tile, c.tile[1] * c.K * 4, out)
        assert tuple(out) == want[c.K]


# ---- conditioning of every summed output of every GPU case -------------------------------------------------------------------------

SUMMED = [c for c in G.all_gpu_cases() if c.summed and c.tier == "highest"]


def test_every_gpu_case_is_listed_once():
    cs = G.all_gpu_cases()
    assert len(set(cs)) == len(cs) and len({(c.name, c.tier) for c in cs}) == len(cs)
    assert {c.epi for c in SUMMED} == {R.EPI_STATS, R.EPI_GEGLU_BWD, R.EPI_SE_RED, R.EPI_ACT_BWD}


@pytest.mark.parametrize("case", SUMMED, ids=lambda c: c.name.replace(" ", "_"))
def test_no_reported_sum_cancels(case):
    """STATS, the ACT_BWD sums, col_sum and SE_RED: |S| >= 0.05 sum|v_i| in every column (SE_RED: every image and column) of the
    fp64 reference.  A sum that cancels measures its inputs' rounding, not the kernel."""
    cond = G.condition(G.reference(case))
    want = {R.EPI_STATS: {"stats"}, R.EPI_ACT_BWD: {"stats"}, R.EPI_GEGLU_BWD: {"col_sum"}, R.EPI_SE_RED: {"C"}}[case.epi]
    assert set(cond) == want
    for name, ratio in cond.items():
        assert ratio >= 0.05, f"{case.name}: {name} cancels to {ratio:.3f} of its terms"
