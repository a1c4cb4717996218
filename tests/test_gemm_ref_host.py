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
