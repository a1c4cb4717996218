"""Per-kernel parity of the contraction family (csrc/gemm_core.hpp, csrc/gemm_dma.hpp, csrc/gemm_split.hpp behind the dispatchers of
csrc/gemm.hip, csrc/gemm_dma.hip and csrc/gemm_split_dispatch.hpp) against tests/gemm_ref.py in fp64 on the CPU (tied to torch autograd
by tests/test_gemm_ref_host.py).  tests/test_gpu_gemm.py stays the full-size leg; here the shapes are the smallest at which each kernel
variant can still go wrong.  The conventions are those of tests/test_gpu_effnet_ops.py: every call goes through lib.gemm = mt_gemm;
stored outputs start as NaN, accumulated ones at a canary that the reference adds; every output is a column slice (leading dimension
N + 8, offset 4) of a tensor whose other columns hold a canary, between -0.0 guard bands; A, B, A2, R and C2 are such slices of
noise-filled tensors (tests/gemm_cases.py); figures are per SECTION -- first / last row tile, first / last column tile, interior, the
worst image of the per-image forms, at the tile size of the variant under test -- and printed (FIG ...) before anything is asserted;
MT_TEST_YARDSTICK=1 prints the same reference evaluated in fp32 torch on the CPU beside them.  Exact checks (guard bands, slice
canaries, untouched rows, refusals, bit-identity, "no NaN left") have no tolerance; the gates are tests/gemm_cases.py TOL.

How each variant is reached, and how that was confirmed from the code:
  * mt_gemm (gemm.hip) asks try_launch_split (gemm_split.hip -> gemm_split_dispatch.hpp launch_split_tier), then try_launch_dma
    (gemm_dma.hip), then launches the register-staged gemm_kernel (gemm_core.hpp) with the tile of pick_cfg.
  * register-staged: launch_split_tier returns 1 for K % 8 != 0 and try_launch_dma for K % 16 != 0 (or M < 64, N < 64), so K 36 / 4092 /
    4100 (K % 8 == 4) and the 4 x 4 x 4 case land in gemm_kernel whatever the pipe.  Prologue calls with K 16 / 40 / 44 get there
    too: try_launch_dma takes prologues only from M >= 4096 and K % 16 == 0, launch_split_tier only from K >= 512 (BN_BWD) or
    M >= 4096 (BN_SWISH_GATE), and neither takes a B prologue.  MT_FORCE_CFG = 0..3 (read per call by pick_cfg) forces the
    128 x 128, 128 x 64, 256 x 32 and 64 x 64 tile; without it N 72 / 68 pad to 128 columns with either width -> 128 x 128;
    N 40 / 136 -> 128 x 64; GEGLU_BWD -> 64 x 64.
  * im2col forms: try_launch_split and try_launch_dma return 1 for MT_PRO_IM2COL and for any B prologue, so every case lands in
    gemm_kernel.  gemm.hip takes the granule form (per-unit window origin + 32-bit tap mask on the A side; per-unit pixel cursor on the
    B side) for an fp32 image with C % 4 == 0 and k k <= 32, else the per-element gather im2col_gather4 (3 channels, uint8, 7 x 7).
    A side: MT_FORCE_CFG = 0..3 as above.  B side (TN, BN_BWD, ATOMIC): Cout <= 64 with 192 < columns <= 288 takes the one-tile
    64 x 288 configuration -- CFG_WG64K (two K groups of six wavefronts), CFG_WG64 in deterministic mode -- with either gather;
    Cout 68 at 288 columns and 192 columns take pick_cfg's 128 x 64, 72 columns 128 x 128, 28 columns 256 x 32.  split_k 3 gives
    K ranges of a multiple of 16 pixels (split_k_ranges), which start inside an image row unless Wo is 16 (test_gemm_ref_host.py
    pins that); split_k 0 is one range below 512 pixels.
  * L2-blocked order: tile_grid (gemm_geometry.hpp) gives group_n > 0 from 32 row tiles and 2 column tiles on; at 64 x 64,
    M 2116 = 34 row tiles (XCD bands of 5, 5, 4, ... rows: padding blocks), N 132 = 3 column tiles, group_n = 2 MB / (64 K 4 B): 2 at
    K 4092 (the last group one tile wide), 1 at K 4100 (test_gemm_ref_host.py pins both through mt_debug_tile_grid).
  * LDS-DMA: the split pipe is off (mt_gemm_set_split(0) makes try_launch_split return 1); M, N >= 64 and K % bk == 0;
    MT_DMA_VARIANT = 0..4 (read per call by pick_variant) picks kVar = (128, 128, 32, 2 stages), (128, 128, 16, 3), (128, 64, 16, 3),
    (64, 64, 32, 3), (64, 64, 16, 3).  The prologue kernels (launch_pro) take NN + BN_BWD with STORE / BIAS_RES / SE_RED / ACT_BWD from
    M >= 4096 at K % 16 == 0; MT_DMA_PRO_VARIANT = 2, 3, 4 picks 128 x 64 (bk 16, 2 stages), 64 x 64 (bk 32, 2 stages: kept only
    for K % 32 == 0, any other K is rewritten to variant 4 -- so variant 3 runs K 32 and 96, the others K 16 and 48) and 64 x 64
    (bk 16, 3 stages).  M 4116 / 4200 are 65 / 66 row tiles of 64 by 2 column tiles: the L2-blocked order again.
  * split-operand loop (pipe on): K % 8 == 0, K >= 512, M >= 128, N >= 64 and M N >= 2^18 -- (1032, 264, 520) with K % 16 == 8 is
    S_BIG (128 x 128), (3656, 72, 512) S_MID (N < 128: 128 x 64) -- or TN with K >= 8192 and M N >= 2^15: (136, 248, 8200).  TN with
    split_k <= 0, K >= 2048 and identity row maps takes the K-range-major XCD form (K_XCD_CAPPED), a given split_k or an a_map the
    plain form.  BN_BWD: NN STORE / BIAS_RES and TN ATOMIC with an identity a_map.  BN_SWISH_GATE: NT from M >= 4096, K >= 256,
    K % 16 == 0; its tile is 128 x 64 only where 64-wide tiles pad fewer columns than 128-wide ones (N 192), else 128 x 128 (N 72).  That the loop ran is proved per case: the result differs in bits from the same call with the pipe off.
  * deterministic mode (det.hip): split-K partial tiles go to slabs that are added in split order (refused for a row-mapped output
    with more than one range: the c_map case has one); col_sum goes through a log that is reduced in rank order."""
import os
from contextlib import contextmanager

import pytest
import torch

from mintime_amd import lib as L

from . import gemm_cases as G
from . import gemm_ref as R
from .gemm_cases import TOL
from .test_gpu_effnet_ops import _Figures, _bands_intact, _det, _guarded, _stats_buffer, _stats_read

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
YARD = bool(os.environ.get("MT_TEST_YARDSTICK"))
F64 = torch.float64


class _Fig(_Figures):
    """_Figures against the gates of tests/gemm_cases.py."""

    def value(self, kind, name, e):
        if self.is_yard:
            print(f"YARD {kind} | {self.what} | {name} | {e:.3e}")
            return e
        print(f"FIG {kind} | {self.what} | {name} | {e:.3e} | tol {TOL[kind]:.0e}")
        if not e <= TOL[kind]:
            self.bad.append(f"{name}: {e:.3e} > {TOL[kind]:.0e}")
        return e


@contextmanager
def _pipe(split, tier):
    prev_s, prev_t = L.set_gemm_split(split), L.set_matmul_precision(tier)
    try:
        yield
    finally:
        L.set_gemm_split(prev_s)
        L.set_matmul_precision(prev_t)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def _launch(case, fig, split=None):
    """One mt_gemm call of the case on fresh buffers.  Returns {name: CPU tensor} of its outputs in logical row order after the exact
    checks: guard bands, every element outside the written slice bit-intact, no NaN left in it."""
    c, b = case, G.inputs(case)
    devt, bufs, stats = {}, {}, None
    for name, w in b.wide.items():
        if name in b.outputs:
            bufs[name], body = _guarded(w.numel())
            body.copy_(w.reshape(-1))
            devt[name] = body.view(w.shape)
        else:
            devt[name] = w.to(dev)
    v = b.views(devt)
    if "stats" in b.outputs:
        bufs["stats"], stats = _stats_buffer(c.slots, c.N)
        v["stats"] = stats
    with _pipe(c.split if split is None else split, c.tier):
        b.call(L.gemm, v, **({"stats_slots": c.slots} if "stats" in b.outputs else {}))
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:       # a device fault: nothing more is started on this card
            pytest.exit(f"{_what(c)}: {e}", returncode=3)
    got = {}
    for name, buf in bufs.items():
        fig.true(f"{name}: guard bands intact", _bands_intact(buf))
    rows = R.map_rows(c.c_map, c.c_rows)
    for name in b.outputs:
        if name == "stats":
            got[name] = _stats_read(stats, c.slots, c.N)
        elif name == "col_sum":
            got[name] = devt[name].cpu()
        else:
            after, before = devt[name].cpu(), b.wide[name]
            written = torch.zeros(before.shape, dtype=torch.bool)
            idx = rows if name == "C" else torch.arange(c.M)
            written[idx, G.OFF:G.OFF + b.cols[name]] = True
            fig.true(f"{name}: nothing outside the output slice was touched", torch.equal(_bits(after)[~written], _bits(before)[~written]))
            got[name] = after[:, G.OFF:G.OFF + b.cols[name]][idx]
            fig.true(f"{name}: no NaN left", not bool(torch.isnan(got[name]).any()))
    if c.bpro == R.BPRO_IM2COL:         # the virtual matrix is exactly zero from k k C on: nothing but +0.0 is ever added there
        pad_cols = got["C"][:, c.taps:]
        fig.true("C: the padding columns keep the canary exactly", torch.equal(_bits(pad_cols), _bits(torch.full_like(pad_cols, G.CANARY))))
    return got


def _high_floors(case, ref):
    """Tier high: per-element bound of C and, for STATS, of the two sums (header bound propagated: d(sum v^2) <= sum 2|v| b + b^2)."""
    if case.tier != "high" or not case.split:
        return None, None, {}
    bound = G.high_bound(case)
    hi = "split."
    tol0 = {k: TOL[hi + k] for k in ("store", "atomic", "fused", "sums")}
    sums = torch.stack((bound.sum(0), (2 * ref["C"].abs() * bound + bound * bound).sum(0))) if case.epi == R.EPI_STATS else None
    return bound, sums, tol0


def _compare(fig, case, got, ref):
    c = case
    bm, bn = c.tile
    bound, sbound, tol0 = _high_floors(c, ref)
    base = c.kind.split(".")[-1]
    kw = dict(floor=bound, tol0=tol0.get(base, 0.0))
    if c.epi == R.EPI_SE_RED:                      # [images, N]: every image is a row; column tiles as usual
        secs = G.sections(got["C"], ref["C"], 1 << 30, bn, hw=1)
    elif c.epi == R.EPI_GEGLU_BWD:                 # the two gradients side by side, each with the tile's sections
        nh = c.n_half
        secs = [(f"{h} {n}", e) for h, s in (("da", slice(0, nh)), ("dg", slice(nh, 2 * nh)))
                for n, e in G.sections(got["C"][:, s], ref["C"][:, s], bm, bn)]
    elif c.epi == R.EPI_GEGLU:                     # a tile of bn weight columns holds bn / 2 columns of h
        secs = G.sections(got["C"], ref["C"], bm, bn // 2)
    else:
        hw = c.e_hw if c.epi == R.EPI_ACT_BWD else (c.hw if c.pro == R.PRO_BN_SWISH_GATE else 0)
        secs = G.sections(got["C"], ref["C"], bm, bn, hw=hw, **kw)
    for n, e in secs:
        fig.value(c.kind, f"C {n}", e)
    skind = c.prefix + "sums"
    if "stats" in ref:
        names = ("sum", "sum of squares") if c.epi == R.EPI_STATS else ("sum du", "sum du xhat")
        for i, nm in enumerate(names):
            for n, e in G.sum_sections(got["stats"][i], ref["stats"][i], bn, None if sbound is None else sbound[i], tol0.get("sums", 0.0)):
                fig.value(skind, f"{nm} (slots {c.slots}) {n}", e)
    if "col_sum" in ref:
        nh = c.n_half
        for h, s in (("da", slice(0, nh)), ("dg", slice(nh, 2 * nh))):
            for n, e in G.sum_sections(got["col_sum"][s], ref["col_sum"][s], bn):
                fig.value(skind, f"col_sum {h} {n}", e)
    if "C2" in ref:
        for n, e in G.sections(got["C2"], ref["C2"], bm, bn):
            fig.value(c.prefix + "store", f"C2 {n}", e)


def _what(c):
    return f"{c.name} | {('NT', 'NN', 'TN')[c.op]} {c.M}x{c.N}x{c.K}" + (f" | tier {c.tier}" if c.split else "")


def _setenv(monkeypatch, case):
    for k in ("MT_FORCE_CFG", "MT_DMA_VARIANT", "MT_DMA_PRO_VARIANT", "MT_SPLIT_PLANES", "MT_DMA_PRO_GATE"):
        monkeypatch.delenv(k, raising=False)
    for k, val in case.env:
        monkeypatch.setenv(k, val)


def _check(case, monkeypatch, figs=None):
    """Launch, print every figure, return the outputs; the caller's fig.done() (or ours) asserts."""
    _setenv(monkeypatch, case)
    ref = G.reference(case)
    if YARD:
        _compare(_Fig(_what(case), True), case, G.reference(case, torch.float32), ref)
    fig = figs if figs is not None else _Fig(_what(case))
    fig.what = _what(case)
    got = _launch(case, fig)
    _compare(fig, case, got, ref)
    return got


def _run(cases, monkeypatch):
    fig = _Fig("")
    for c in cases:
        _check(c, monkeypatch, fig)
    fig.done()


# ---- (a) register-staged kernels ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_register_staged_tiles(cfg, monkeypatch):
    """The four tiles of gemm_kernel, forced by MT_FORCE_CFG: three row tiles by two column tiles with 4-row / 4-column last tiles,
    one exact tile, and 4 x 4 x 4; NT STORE + bias, NT BIAS_RES in place, NT STATS, NN STORE, NN ACCUM, TN ATOMIC (1 and 3 K ranges)."""
    _run(G.cfg_cases(cfg), monkeypatch)


def test_l2_blocked_tile_order(monkeypatch):
    """tile_coords with group_n > 0 and padding blocks (module docstring): every tile is computed once, nothing else is written."""
    _run(G.l2_cases(), monkeypatch)


@pytest.mark.parametrize("hw", [1, 9, 49])
def test_gate_prologue_small(hw, monkeypatch):
    """NT BN_SWISH_GATE (STORE, STATS) below M 4096 with image boundaries inside a tile."""
    _run(G.gate_pro_cases(hw), monkeypatch)


@pytest.mark.parametrize("K", [36, 40, 44])
def test_bn_bwd_prologue_k_tail(K, monkeypatch):
    """NN BN_BWD (STORE, BIAS_RES) and TN BN_BWD (ATOMIC) with a partial last k-tile: kc stays out of the zero-filled tail."""
    _run(G.bn_bwd_cases(K), monkeypatch)


@pytest.mark.parametrize("b_hw", [1, 9, 49])
def test_b_prologue_weight_gradient(b_hw, monkeypatch):
    """TN BN_BWD + BPRO_BN_SWISH_GATE: the project conv's weight gradient below 100 000 rows and in deterministic mode."""
    _run(G.bpro_cases(b_hw), monkeypatch)


@pytest.mark.parametrize("e_hw", [1, 5, 49, 200])
def test_se_epilogues_register_staged(e_hw, monkeypatch):
    """SE_RED and ACT_BWD (fp64 slots and integer limbs) with images shorter than the lane stride, several per tile, and longer than
    a tile; rows past the last image of SE_RED's output stay untouched."""
    _run(G.se_cases(e_hw), monkeypatch)


def test_act_bwd_integer_limb_sums_are_bit_reproducible(monkeypatch):
    case = [c for c in G.se_cases(49) if c.epi == R.EPI_ACT_BWD and c.slots < 0][0]
    _setenv(monkeypatch, case)
    fig = _Fig(_what(case))
    a, b = _launch(case, fig), _launch(case, fig)
    fig.true("two launches give the same limb sums", torch.equal(_bits(a["stats"]), _bits(b["stats"])))
    fig.true("two launches give the same du", torch.equal(_bits(a["C"]), _bits(b["C"])))
    fig.done()


@pytest.mark.parametrize("n_half", [64, 192])
def test_geglu_bwd_nt_and_nn(n_half, monkeypatch):
    """GEGLU_BWD over the transposed weight (NT) and over the weight (NN), ldc = ldc2 = 2 n_half + 8, col_sum on a canary."""
    _run(G.geglu_bwd_cases(n_half), monkeypatch)


# ---- (a') the im2col forms of the register-staged kernels ---------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_im2col_forward(cfg, monkeypatch):
    """MT_PRO_IM2COL with STORE and STATS on each of the four tiles: the granule form (window origin + tap mask per unit) and the
    per-element gather (3 channels, uint8, k k > 32), over images with H != W, windows that hang over the bottom / right edge,
    padding >= k, a strided 1 x 1 and K up to 576; the image is a dense tensor inside a noise-filled allocation, the packed weights
    hold noise in their padding columns (tests/gemm_cases.py IM2COL_A)."""
    _run(G.im2col_a_cases(cfg), monkeypatch)


IM2COL_B_GROUPS = sorted({g[0] for g in G.IM2COL_B})


@pytest.mark.parametrize("group", IM2COL_B_GROUPS)
def test_im2col_weight_gradient(group, monkeypatch):
    """MT_BPRO_IM2COL (TN, BN_BWD on A, ATOMIC onto a canary) at split_k 1, 3 and auto: the granule form's pixel cursor across image
    rows shorter than, equal to and longer than the k-step, across images and from a K range that starts inside a row; the one-tile
    64 x 288 configuration (CFG_WG64K here, CFG_WG64 in deterministic mode) and the shapes just outside it; the per-element gather
    over fp32 and uint8 crops (tests/gemm_cases.py IM2COL_B)."""
    _run([c for c in G.im2col_b_cases() if c.name.startswith(f"im2col wgrad {group} ")], monkeypatch)


# ---- (b) LDS-DMA kernels -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_dma_variants_ring_depths(variant, monkeypatch):
    """K = bk, 2 bk, (stages + 1) bk at (bm + 4, bn + 4) and (64, 64): NT STORE + bias, NN STORE, TN ATOMIC with two K ranges."""
    _run(G.dma_cases(variant), monkeypatch)


@pytest.mark.parametrize("variant", [2, 3, 4])
def test_dma_prologue_se_epilogues(variant, monkeypatch):
    """SE_RED and ACT_BWD on the LDS-DMA prologue kernels at M >= 4096."""
    _run(G.dma_pro_cases(variant), monkeypatch)


# ---- (c) split-operand loop --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tier", ["highest", "high"])
def test_split_operand_loop(tier, monkeypatch):
    fig = _Fig("")
    for c in G.split_cases(tier):
        got = _check(c, monkeypatch, fig)
        other = _launch(c, fig, split=False)
        fig.true("the split loop ran: bits differ from the fp32 pipe's", not torch.equal(_bits(got["C"]), _bits(other["C"])))
    fig.done()


def test_other_launchable_forms(monkeypatch):
    """tests/gemm_cases.py extra_cases: what gemm.hip, gemm_dma.hip and gemm_split_dispatch.hpp can launch beyond the lists above."""
    fig = _Fig("")
    for c in G.extra_cases():
        got = _check(c, monkeypatch, fig)
        if c.split:
            other = _launch(c, fig, split=False)
            fig.true("the split loop ran: bits differ from the fp32 pipe's", not torch.equal(_bits(got["C"]), _bits(other["C"])))
    fig.done()


# ---- (d) deterministic mode --------------------------------------------------------------------------------------------------------

def _det_groups():
    a = [c for cfg in range(4) for c in G.cfg_cases(cfg)] + [c for K in (36, 40, 44) for c in G.bn_bwd_cases(K)]
    a += [c for h in (1, 9, 49) for c in G.bpro_cases(h)]
    groups = {"register-staged": a, "dma": [c for v in range(5) for c in G.dma_cases(v)], "split-highest": G.split_cases("highest"),
              "split-high": G.split_cases("high")}
    groups["other forms"] = G.extra_cases()
    for g in IM2COL_B_GROUPS:
        groups[f"im2col wgrad {g}"] = [c for c in G.im2col_b_cases() if c.name.startswith(f"im2col wgrad {g} ")]
    groups = {k: [c for c in v if c.epi == R.EPI_ATOMIC] for k, v in groups.items()}
    groups["geglu_bwd"] = [c for nh in (64, 192) for c in G.geglu_bwd_cases(nh)]
    return groups


DET = _det_groups()


@pytest.mark.parametrize("group", sorted(DET))
def test_deterministic_mode(group, monkeypatch):
    """Every ATOMIC case (the row-mapped one included) and the col_sum of GEGLU_BWD with mt_set_deterministic(1): two launches agree
    in every bit, the result passes the same gates, bands and canaries are intact."""
    fig = _Fig("")
    with _det(True):
        for c in DET[group]:
            first = _check(c, monkeypatch, fig)
            again = _launch(c, fig)
            for name in first:
                fig.true(f"{name}: two deterministic launches agree in every bit", torch.equal(_bits(first[name]), _bits(again[name])))
    fig.done()


# ---- (e) refusals ------------------------------------------------------------------------------------------------------------------

MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3          # csrc/common.hpp


def _refused(code, op, M, N, K, lda, ldb, a_off=0, **kw):
    """The call raises with `code` and leaves the NaN-filled, guarded output as it was."""
    A = torch.ones(64 * 64 + 8, device=dev)[a_off:]
    B = torch.ones(64 * 64, device=dev)
    buf, C = _guarded(64 * 64)
    before = buf.clone()
    with pytest.raises(L.MintimeHipError, match=rf"failed \({code}\)"):
        L.gemm(op, A, B, C, M, N, K, lda, ldb, 64, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(before))


def test_refusals_launch_nothing():
    vec = torch.ones(64, device=dev)
    z = torch.ones(64 * 64, device=dev)
    bn = dict(prologue=L.PRO_BN_BWD, scale=vec, shift=vec, gate=vec, A2=z)
    e5 = (vec, vec, z, z, torch.ones(128, device=dev), 4)
    _refused(MT_ERR_ARG, L.OP_NT, 16, 16, 6, 8, 8)                                                  # NT: K % 4
    _refused(MT_ERR_ARG, L.OP_NN, 16, 18, 8, 8, 20)                                                 # NN: N % 4
    _refused(MT_ERR_ARG, L.OP_TN, 18, 16, 8, 20, 16, epilogue=L.EPI_ATOMIC)                         # TN: M % 4
    _refused(MT_ERR_ARG, L.OP_NT, 16, 16, 8, 10, 8)                                                 # lda % 4
    _refused(MT_ERR_ARG, L.OP_NT, 16, 16, 8, 8, 8, a_off=1)                                         # A not 16-byte aligned
    _refused(MT_ERR_ARG, L.OP_NN, 16, 16, 8, 8, 16, epilogue=L.EPI_SE_RED, epi=e5, **bn)            # SE_RED without C2
    _refused(MT_ERR_ARG, L.OP_NN, 16, 16, 8, 8, 16, epilogue=L.EPI_ACT_BWD, epi=e5, C2=z, ldc2=16, **bn)         # ACT_BWD without stats
    _refused(MT_ERR_ARG, L.OP_NN, 16, 16, 8, 8, 16, epilogue=L.EPI_SE_RED, epi=e5, C2=z, ldc2=16, c_map=(4, 5, 1), **bn)
    _refused(MT_ERR_UNSUPPORTED, L.OP_NT, 16, 16, 8, 8, 8, epilogue=L.EPI_SE_RED, epi=e5, C2=z, ldc2=16, **bn)   # SE_RED on NT
    _refused(MT_ERR_ARG, L.OP_NT, 16, 16, 8, 8, 8, b_prologue=L.BPRO_BN_SWISH_GATE, b_scale=vec, b_shift=vec, b_gate=z, b_hw=4)
    _refused(MT_ERR_ARG, L.OP_NT, 16, 64, 8, 8, 8, epilogue=L.EPI_GEGLU, n_half=32, C2=z, ldc2=64)  # GEGLU: n_half % 64
    # the im2col forms: one 8 x 8 x 4 image, 3 x 3 at pad 1 -> 64 pixels by 36 columns; the forward as NT 64 x 16 x 36, the weight
    # gradient as TN 16 x 36 x 64
    geo = (8, 8, 4, 8, 8, 3, 1, 1, 0)
    fwd = lambda code, K=36, **kw: _refused(code, L.OP_NT, 64, 16, K, K, K, **{"prologue": L.PRO_IM2COL, "conv": geo, **kw})
    wg = lambda code, op=L.OP_TN, N=36, **kw: _refused(code, op, 16, N, 64, 16, N, **{"b_prologue": L.BPRO_IM2COL, "conv": geo,
                                                                                    "epilogue": L.EPI_ATOMIC, **bn, **kw})
    fwd(MT_ERR_UNSUPPORTED, conv=geo + (1,))                                                        # a uint8 source with C % 4 == 0
    wg(MT_ERR_UNSUPPORTED, conv=geo + (1,))
    wg(MT_ERR_ARG, op=L.OP_NT)                                                                      # B prologue on anything but TN
    wg(MT_ERR_ARG, op=L.OP_NN)
    wg(MT_ERR_UNSUPPORTED, prologue=L.PRO_NONE)                                                     # ... without BN_BWD on A
    wg(MT_ERR_UNSUPPORTED, epilogue=L.EPI_STORE)                                                    # ... into anything but ATOMIC
    for e in (L.EPI_ATOMIC, L.EPI_ACCUM, L.EPI_BIAS_RES):                                           # A prologue: STORE / STATS only
        fwd(MT_ERR_UNSUPPORTED, epilogue=e, R=z, ldr=64)
    fwd(MT_ERR_ARG, conv=None)                                                                      # no geometry
    fwd(MT_ERR_ARG, conv=(8, 8, 4, 8, 8, 0, 1, 1, 0))
    wg(MT_ERR_ARG, conv=(8, 8, 4, 8, 0, 3, 1, 1, 0))
    fwd(MT_ERR_ARG, scale=vec)                                                                      # a scale without a shift
    fwd(MT_ERR_ARG, shift=vec)
    wg(MT_ERR_ARG, b_scale=vec)
    fwd(MT_ERR_ARG, conv=(0, 8, 4, 8, 8, 3, 1, 1, 0))                                               # an image without rows / columns
    fwd(MT_ERR_ARG, conv=(8, -8, 4, 8, 8, 3, 1, 1, 0))
    wg(MT_ERR_ARG, conv=(8, 0, 4, 8, 8, 3, 1, 1, 0))
    fwd(MT_ERR_ARG, K=32)                                                                           # fewer columns than k k C = 36
    wg(MT_ERR_ARG, N=32)
