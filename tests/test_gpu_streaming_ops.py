"""Per-kernel parity of the streaming 1x1 convolution kernels of the EfficientNet extractor (csrc/skinny_conv.hip, skinny_wgrad.hip,
skinny_bwd.hip, skinny_se.hip, wide_wgrad.hip: mt_conv1x1_rows, mt_conv1x1_wgrad, mt_conv1x1_wgrad_wide, mt_conv1x1_bwd_fused,
mt_se_stage_fused) against tests/streaming_ops_ref.py in fp64 on the CPU (tied to torch autograd, with the case tables' branch
reach, by tests/test_streaming_ops_ref_host.py).  Conventions of tests/test_gpu_effnet_ops.py: every test calls the C ABI; stored
outputs start as NaN, accumulated ones (dw, dgate) at a canary that the reference adds; outputs and statistics sit between -0.0 guard
bands; every INPUT sits between NaN guard bands and the pad columns of a pitched weight hold NaN, so a clamped load that leaks
poisons a figure; figures are printed before anything is asserted; comparisons are per section (streaming_ops_ref.row_sections,
col_sections, image_sections).

Gates.  For every case and section the yardstick is the same reference function evaluated in fp32 torch on the CPU, compared with
fp64, computed at test time (MT_TEST_YARDSTICK=1 prints it beside the kernel's figure); the gate of a section is
min(ceiling, max(1e-6, 5 x yardstick)) with the project's ceilings (_CEILING of test_gpu_effnet_ops.py: 2e-5 stored data, 1e-4 sums,
GRAD_TOL_UNIT weight gradients).  Keys of TOL override it where a kernel's accumulation order, not an error, explains the figure.
The exact checks (guard bands, no NaN, exact zeros, bit-identity of single-writer outputs and of integer-limb sums over two launches,
refusals with untouched outputs) have no tolerance.  Measured on an MI355X (worst figure / its gate / its yardstick, case):
  rows.out   3.0e-7 / 1.5e-6 / 3.0e-7   96 -> 16 gated, rows 385, hw 128, last partial column tile
  rows.sums  4.6e-7 / 1e-6   / 1.5e-7   4 -> 1, one row, sum out^2 (fp64 slot)
  wgrad.dw   1.0e-6 / 2e-6   / 3.9e-7   44 x 12 plain, rows 32841, last partial column tile (fp32 atomics: moves by ~2e-7 between runs)
  wide.dw    5.4e-7 / 2e-6   / 3.9e-7   164 x 240, rows 18451, hw 49, last slab
  fused.dx   5.0e-7 / 2.2e-6 / 4.4e-7   96 -> 16, rows 24513, residual, later chunks of a block
  fused.dw   6.2e-7 / 2.9e-6 / 5.8e-7   96 -> 16, rows 73727
  se.dgate   1.9e-7 / 1e-6   / 1.6e-7   144 -> 24, hw 64, 2 images, image 0
  se.du_d    2.5e-7 / 1.3e-6 / 2.5e-7   96 -> 32, hw 192, 200 images
  se.sums    1.9e-7 / 1.5e-6 / 2.9e-7   32 -> 32, hw 64, 3 images, sum du_d xhat
The largest kernel / yardstick ratio is 4.3 (rows kernel, one row, K = 4: 2.5e-7 against 5.8e-8, under the floor), then 2.9 (wgrad.dw, 52 x 108 gated, rows 16425: 8.3e-7 / 2.9e-7).

How each branch is reached is stated in streaming_ops_ref.py beside the tables and asserted by test_streaming_ops_ref_host.py from the
launch geometry read off the launchers: mt_conv1x1_rows 128-row chunks, min(chunks, 512) blocks, block b walks b, b + grid, ...;
mt_conv1x1_wgrad 128 / 64 / 32-row chunks per instance, min(chunks, 256 * BPC) blocks, strided; mt_conv1x1_bwd_fused 64-row chunks,
min(chunks, CUs) blocks, strided; mt_se_stage_fused 64-row chunks, min(chunks, 512) blocks, contiguous ranges of ceil(chunks / grid);
mt_conv1x1_wgrad_wide 32-row chunks, 8 * max(1, CUs / (8 * slabs)) row ranges (rounded down to the chunks), contiguous.  Where the CU
count enters, the table is a function of it and the test takes it from the device.  Cout 33 of mt_conv1x1_rows has no instance (two
column tiles): it is pinned as a refusal and Cout 65 is the scalar-epilogue case of the three-tile instance."""
import os

import pytest
import torch

from mintime_amd import lib as L

from . import streaming_ops_ref as R
from .test_gpu_effnet_ops import _CEILING, _bands_intact, _guarded, _stats_buffer, _stats_read
from .util import GRAD_TOL_UNIT, rel_err

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
CANARY = 7.0
NAN = float("nan")
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3          # csrc/common.hpp
YARD = bool(os.environ.get("MT_TEST_YARDSTICK"))
F64 = torch.float64

CEILING = {"out": _CEILING["data"], "dx": _CEILING["data"], "du_d": _CEILING["data"], "sums": _CEILING["sums"], "dgate": _CEILING["sums"],
           "dw": GRAD_TOL_UNIT}
# key -> gate, for the keys whose figure follows from the accumulation order (none unless listed; see the module docstring)
TOL = {}
assert all(v <= CEILING[k.split(".")[-1]] for k, v in TOL.items())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nz(g, *shape, scale=1.0):
    """Non-zero, distinct values: +-(0.5 .. 1.5) * scale."""
    sign = torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    return sign * (torch.rand(*shape, generator=g) + 0.5) * scale


def _in(t):
    """An input on the device between two 64-element bands of NaN (16-byte alignment kept)."""
    if t is None:
        return None
    buf = torch.full((t.numel() + 128,), NAN, device=dev)
    body = buf[64:64 + t.numel()].view(t.shape)
    body.copy_(t)
    return body


def _f64(*ts):
    return [None if t is None else t.double() for t in ts]


class _Figures:
    """One test's figures: each is printed with its yardstick and gate before anything is asserted; done() fails on all that missed."""

    def __init__(self, what):
        self.what, self.bad, self.worst = what, [], {}

    def close(self, key, name, got, ref, yard):
        got = got.detach().cpu().double()
        e, y = rel_err(got, ref), rel_err(yard, ref)
        gate = TOL.get(key, min(CEILING[key.split(".")[-1]], max(1e-6, 5 * y)))
        print(f"FIG {key} | {self.what} | {name} | {e:.3e} | gate {gate:.1e}" + (f" | yard {y:.3e} | ratio {e / max(y, 1e-30):.2f}" if YARD else ""))
        if not e <= gate:
            self.bad.append(f"{name}: {e:.3e} > {gate:.1e} (yardstick {y:.3e})")
        return e

    def true(self, name, cond):
        if not bool(cond):
            print(f"FIG exact | {self.what} | {name} | FALSE")
            self.bad.append(name)

    def done(self):
        assert not self.bad, f"{self.what}: " + "; ".join(self.bad)


def _cmp(fig, key, name, got, ref, yard, dim0=(), dim1=()):
    """Whole tensor, then the sections along dim 0 and dim 1; exact zeros of the reference must be exact in `got`."""
    got = got.detach().cpu()
    fig.true(f"{name} has no NaN", not bool(torch.isnan(got).any()))
    fig.close(key, name, got, ref, yard)
    for n, i in dim0:
        if not (n.endswith("all")):
            fig.close(key, f"{name} [{n}]", got[i], ref[i], yard[i])
    for n, i in dim1:
        fig.close(key, f"{name} [{n}]", got[..., i], ref[..., i], yard[..., i])


def _exact_zeros(fig, name, got, ref_without_fill, fill=0.0):
    m = ref_without_fill == 0
    fig.true(f"{name}: exact zeros of the reference are exact ({int(m.sum())})", (got.detach().cpu()[m] == fill).all())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. mt_conv1x1_rows ----------------------------------------------------------------------------------------------------------------


def _rows_launch(d, wbuf, ldw, wt, amode, hw, rows, Cin, Cout, slots):
    obuf, out = _guarded(rows * Cout)
    sbuf, st = _stats_buffer(slots, Cout) if slots else (None, None)
    L.check(L.get().mt_conv1x1_rows(L.ptr(d["x"]), L.ptr(d["x2"]), L.ptr(wbuf), ldw, wt, L.ptr(d["c0"]), L.ptr(d["c1"]), L.ptr(d["c2"]), hw,
                                    amode, L.ptr(d["res"]), L.ptr(out), L.ptr(st), slots, rows, Cin, Cout, L.stream_ptr()), "mt_conv1x1_rows")
    torch.cuda.synchronize()
    assert _bands_intact(obuf) and (sbuf is None or _bands_intact(sbuf)), "mt_conv1x1_rows wrote outside its outputs"
    return out.view(rows, Cout), st


@pytest.mark.parametrize("Cin,Cout,amode,rows,hw,pad,wt,with_res,forms", R.ROWS_CASES)
def test_conv1x1_rows_vs_fp64(Cin, Cout, amode, rows, hw, pad, wt, with_res, forms):
    """out per section, the column sums and sums of squares in every statistics form of the case (0 = none, fp64 slots, integer limbs
    decoded as stat_get does), out bit-identical across forms and launches, limb sums bit-identical over two launches."""
    g = _gen(Cin * 1000 + Cout * 10 + amode)
    x = torch.randn(rows, Cin, generator=g)
    x2 = torch.randn(rows, Cin, generator=g) if amode == 2 else None
    W = torch.randn(Cout, Cin, generator=g) * 0.3 + 0.05
    if Cout > 1:
        W[Cout - 1] = 0.0                                           # an output column that is exactly 0 (+ res)
    wbuf = torch.full((Cin, Cout + pad) if wt else (Cout, Cin + pad), NAN)
    if wt:
        wbuf[:, :Cout] = W.t()
    else:
        wbuf[:, :Cin] = W
    c0 = c1 = c2 = None
    if amode == 1:
        c0, c1, c2 = _nz(g, Cin), _nz(g, Cin, scale=0.3), torch.rand(R.cdiv(rows, hw), Cin, generator=g) + 0.25
    elif amode == 2:
        c0, c1, c2 = _nz(g, Cin), _nz(g, Cin, scale=0.3), _nz(g, Cin, scale=0.1)
    res = torch.randn(rows, Cout, generator=g) if with_res else None
    ref = R.conv1x1_rows(x.double(), wbuf.double(), wt, Cout, amode, *_f64(x2, c0, c1, c2), hw, None if res is None else res.double())
    yard = R.conv1x1_rows(x, wbuf, wt, Cout, amode, x2, c0, c1, c2, hw, res)
    d = {k: _in(v) for k, v in dict(x=x, x2=x2, c0=c0, c1=c1, c2=c2, res=res).items()}
    wd, ldw = _in(wbuf), wbuf.shape[1]
    fig = _Figures(f"rows {Cin}->{Cout} mode {amode} rows {rows} hw {hw} ldw {ldw} wt {wt} res {int(with_res)}")
    walk = R.rows_walk(rows)
    first = None
    for slots in forms:
        out, st = _rows_launch(d, wd, ldw, wt, amode, hw, rows, Cin, Cout, slots)
        out2, st2 = _rows_launch(d, wd, ldw, wt, amode, hw, rows, Cin, Cout, slots)
        fig.true(f"out is the same bits over two launches (slots {slots})", _same_bits(out, out2))
        if first is None:
            first = out
            _cmp(fig, "rows.out", "out", out, ref[0], yard[0], R.row_sections(walk), R.col_sections(Cout))
            _exact_zeros(fig, "out", out, ref[0])
        else:
            fig.true(f"out is the same bits in every statistics form (slots {slots})", _same_bits(out, first))
        if slots:
            got = _stats_read(st, slots, Cout)
            fig.true(f"sums have no NaN (slots {slots})", not bool(torch.isnan(got).any()))
            _cmp(fig, "rows.sums", f"sum out (slots {slots})", got[0], ref[1], yard[1], dim1=R.col_sections(Cout))
            _cmp(fig, "rows.sums", f"sum out^2 (slots {slots})", got[1], ref[2], yard[2], dim1=R.col_sections(Cout))
            if slots < 0:
                fig.true(f"limb sums are the same bits over two launches (slots {slots})", torch.equal(st.view(torch.int64), st2.view(torch.int64)))
    fig.done()


# ---- 2. mt_conv1x1_wgrad / mt_conv1x1_wgrad_wide ----------------------------------------------------------------------------------------


def _wgrad_check(fn, Cout, Cin, rows, hw, slab=None):
    g = _gen(Cout * 1000 + Cin + rows % 97)
    du, z = torch.randn(rows, Cout, generator=g), torch.randn(rows, Cout, generator=g)
    kabc = torch.stack([_nz(g, Cout), _nz(g, Cout, scale=0.3), _nz(g, Cout, scale=0.1)])
    x = torch.randn(rows, Cin, generator=g)
    sc = sh = gate = None
    if hw:
        sc, sh, gate = _nz(g, Cin), _nz(g, Cin, scale=0.3), torch.rand(R.cdiv(rows, hw), Cin, generator=g) + 0.25
        gate[:, 1] = 0.0                                           # a weight-gradient column that stays exactly at the canary
    else:
        x[:, 1] = 0.0
    args64 = _f64(du, z, kabc, x, sc, sh, gate)
    ref0 = R.conv1x1_wgrad(*args64, hw or 1)
    ref = ref0 + CANARY
    yard = R.conv1x1_wgrad(du, z, kabc, x, sc, sh, gate, hw or 1, CANARY)
    d = [_in(t) for t in (du, z, kabc, x, sc, sh, gate)]
    dbuf, dw = _guarded(Cout * Cin, CANARY)
    L.check(getattr(L.get(), fn)(*[L.ptr(t) for t in d], hw, L.ptr(dw), rows, Cout, Cin, L.stream_ptr()), fn)
    torch.cuda.synchronize()
    fig = _Figures(f"{fn} {Cout}x{Cin} rows {rows} hw {hw}")
    fig.true("guard bands intact", _bands_intact(dbuf))
    dw = dw.view(Cout, Cin)
    _cmp(fig, "wgrad.dw" if slab is None else "wide.dw", "dw", dw, ref, yard, R.col_sections(Cout), R.col_sections(Cin, slab))
    _exact_zeros(fig, "dw", dw, ref0, CANARY)
    fig.done()


@pytest.mark.parametrize("Cout,Cin,rows,hw", R.WGRAD_CASES)
def test_conv1x1_wgrad_vs_fp64(Cout, Cin, rows, hw):
    """Every one of the 18 instances at channel counts that are no multiples of 32, plain and gated (hw 1, 7, 49, the chunk height,
    above rows), rows 1 / R - 1 / R + 1, and per chunk height and row-group arrangement one case whose blocks walk two chunks."""
    _wgrad_check("mt_conv1x1_wgrad", Cout, Cin, rows, hw)


@pytest.mark.parametrize("case", range(len(R.wide_cases(256))))
def test_conv1x1_wgrad_wide_vs_fp64(case):
    """All four Co tile counts, 2 .. 16 slabs (partial, 32 wide), hw 32 / 49 / 196, 1 .. 5 chunks per split from the CU count."""
    Cout, Cin, rows, hw, _ = R.wide_cases(_cus())[case]
    _wgrad_check("mt_conv1x1_wgrad_wide", Cout, Cin, rows, hw, slab=128)


# ---- 3. mt_conv1x1_bwd_fused -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", range(len(R.fused_cases(256))))
def test_conv1x1_bwd_fused_vs_fp64(case):
    """dx per section (single writer: bit-identical over two launches) and dw on its canary, against the unfolded fp64 form."""
    cus = _cus()
    Cout, Cin, rows, with_res = R.fused_cases(cus)[case]
    g = _gen(Cout * 100 + Cin + case)
    du, x = torch.randn(rows, Cout, generator=g), torch.randn(rows, Cin, generator=g)
    x[:, 1] = 0.0                                                  # dw[:, 1] stays exactly at the canary
    W = torch.randn(Cout, Cin, generator=g) * 0.2
    kabc = torch.stack([_nz(g, Cout), _nz(g, Cout, scale=0.3), _nz(g, Cout, scale=0.1)])
    res = torch.randn(rows, Cin, generator=g) if with_res else None
    ref = R.conv1x1_bwd_fused(*_f64(du, kabc, x, W, res))
    yard = R.conv1x1_bwd_fused(du, kabc, x, W, res)
    d = [_in(t) for t in (du, kabc, x, W, res)]
    fig = _Figures(f"bwd_fused {Cout}->{Cin} rows {rows} res {int(with_res)} cus {cus}")
    outs = []
    for _ in range(2):
        xbuf, dx = _guarded(rows * Cin)
        wbuf, dw = _guarded(Cout * Cin, CANARY)
        L.check(L.get().mt_conv1x1_bwd_fused(*[L.ptr(t) for t in d], L.ptr(dx), L.ptr(dw), rows, Cout, Cin, L.stream_ptr()), "mt_conv1x1_bwd_fused")
        torch.cuda.synchronize()
        fig.true("guard bands intact", _bands_intact(xbuf) and _bands_intact(wbuf))
        outs.append((dx.view(rows, Cin), dw.view(Cout, Cin)))
    dx, dw = outs[0]
    fig.true("dx is the same bits over two launches", _same_bits(dx, outs[1][0]))
    _cmp(fig, "fused.dx", "dx", dx, ref[0], yard[0], R.row_sections(R.fused_walk(rows, cus)), R.col_sections(Cin))
    _cmp(fig, "fused.dw", "dw", dw, ref[1] + CANARY, yard[1] + CANARY, dim1=R.col_sections(Cin))
    _exact_zeros(fig, "dw", dw, ref[1], CANARY)
    fig.done()


# ---- 4. mt_se_stage_fused ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("Co,C,hw,n_img,forms", R.SE_CASES)
def test_se_stage_fused_vs_fp64(Co, C, hw, n_img, forms):
    """Mode 0: dgate on its canary, whole and for the first, a middle and the last image.  Mode 1: du_d per section (bit-identical over
    two launches) and both BatchNorm-backward sums by value in fp64 slots and integer limbs (limbs bit-identical over two launches)."""
    rows = n_img * hw
    g = _gen(Co * 1000 + C + hw)
    du, zp = torch.randn(rows, Co, generator=g), torch.randn(rows, Co, generator=g)
    kabc = torch.stack([_nz(g, Co), _nz(g, Co, scale=0.3), _nz(g, Co, scale=0.1)])
    W = torch.randn(Co, C, generator=g) * 0.2
    W[:, 1] = 0.0                                                  # da[:, 1] = 0: dgate[:, 1] stays exactly at the canary
    zd = torch.randn(rows, C, generator=g)
    scale, shift = torch.rand(C, generator=g) + 0.5, _nz(g, C, scale=0.3)
    gate, dpool = torch.rand(n_img, C, generator=g) + 0.25, torch.randn(n_img, C, generator=g)
    mi = torch.stack([_nz(g, C, scale=0.2), torch.rand(C, generator=g) + 0.5])
    base = (du, zp, kabc, W, zd, scale, shift)
    d = [_in(t) for t in base]
    gd, pd, md = _in(gate), _in(dpool), _in(mi)
    lib, fig = L.get(), _Figures(f"se_stage {C}->{Co} hw {hw} images {n_img}")
    walk = R.se_walk(rows)

    ref0 = R.se_stage(*_f64(*base), 0, hw)[0]
    yard0 = R.se_stage(*base, 0, hw, dgate0=CANARY)[0]
    gbuf, dgate = _guarded(n_img * C, CANARY)
    L.check(lib.mt_se_stage_fused(*[L.ptr(t) for t in d], 0, L.ptr(dgate), None, None, None, None, None, 1, rows, Co, C, hw, L.stream_ptr()),
            "mt_se_stage_fused mode 0")
    torch.cuda.synchronize()
    fig.true("guard bands intact (mode 0)", _bands_intact(gbuf))
    dgate = dgate.view(n_img, C)
    _cmp(fig, "se.dgate", "dgate", dgate, ref0 + CANARY, yard0, R.image_sections(n_img), R.col_sections(C))
    _exact_zeros(fig, "dgate", dgate, ref0, CANARY)

    ref1 = R.se_stage(*_f64(*base), 1, hw, *_f64(gate, dpool, mi))
    yard1 = R.se_stage(*base, 1, hw, gate, dpool, mi)
    first = None
    for slots in forms:
        runs = []
        for _ in range(2):
            ubuf, dud = _guarded(rows * C)
            sbuf, st = _stats_buffer(slots, C)
            L.check(lib.mt_se_stage_fused(*[L.ptr(t) for t in d], 1, None, L.ptr(gd), L.ptr(pd), L.ptr(md), L.ptr(dud), L.ptr(st), slots, rows,
                                          Co, C, hw, L.stream_ptr()), "mt_se_stage_fused mode 1")
            torch.cuda.synchronize()
            fig.true(f"guard bands intact (mode 1, slots {slots})", _bands_intact(ubuf) and _bands_intact(sbuf))
            runs.append((dud.view(rows, C), st))
        dud, st = runs[0]
        fig.true(f"du_d is the same bits over two launches (slots {slots})", _same_bits(dud, runs[1][0]))
        if first is None:
            first = dud
            _cmp(fig, "se.du_d", "du_d", dud, ref1[0], yard1[0], R.row_sections(walk), R.col_sections(C))
        else:
            fig.true(f"du_d is the same bits in every statistics form (slots {slots})", _same_bits(dud, first))
        got = _stats_read(st, slots, C)
        _cmp(fig, "se.sums", f"sum du_d (slots {slots})", got[0], ref1[1], yard1[1], dim1=R.col_sections(C))
        _cmp(fig, "se.sums", f"sum du_d xhat (slots {slots})", got[1], ref1[2], yard1[2], dim1=R.col_sections(C))
        if slots < 0:
            fig.true(f"limb sums are the same bits over two launches (slots {slots})",
                     torch.equal(st.view(torch.int64), runs[1][1].view(torch.int64)))
    fig.done()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------


class _Refusals:
    """Calls that must be refused on the host before any launch: the return code, mt_last_error naming the entry point, and every
    output still at its fill afterwards."""

    def __init__(self, name):
        self.name, self.fn, self.outs, self.n = name, getattr(L.get(), name), [], 0

    def buf(self, numel, fill=0.0, dtype=torch.float32, out=False):
        t = torch.full((numel,), fill, dtype=dtype, device=dev)
        if out:
            self.outs.append((t, fill))
        return t

    def refuse(self, code, *args):
        rc = self.fn(*[L.ptr(a) if torch.is_tensor(a) else a for a in args], L.stream_ptr())
        msg = (L.get().mt_last_error() or b"").decode()
        assert rc == code, f"{self.name}{args[-6:]}: returned {rc}, expected {code} ({msg})"
        assert msg.startswith(self.name + ":"), msg
        self.n += 1

    def done(self, at_least):
        torch.cuda.synchronize()
        assert self.n >= at_least
        for t, fill in self.outs:
            assert bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all()), f"{self.name}: a refused call wrote an output"


def _off(t):
    return t[1:]           # the same buffer 4 bytes on: not 16-byte aligned


def test_conv1x1_rows_refusals():
    r = _Refusals("mt_conv1x1_rows")
    x, x2, w, c0, c1, c2, res = [r.buf(1 << 14) for _ in range(7)]
    out, st = r.buf(1 << 14, NAN, out=True), r.buf(1 << 12, 0.0, F64, out=True)

    def call(code, x=x, x2=None, w=w, c0=None, c1=None, c2=None, hw=1, amode=0, out=out, rows=64, Cin=16, Cout=96):
        r.refuse(code, x, x2, w, Cin, 0, c0, c1, c2, hw, amode, res, out, st, 8, rows, Cin, Cout)

    call(MT_ERR_ARG, x=None), call(MT_ERR_ARG, w=None), call(MT_ERR_ARG, out=None)
    call(MT_ERR_ARG, rows=0), call(MT_ERR_ARG, rows=-5)
    for Cin, Cout in ((16, 33), (16, 64), (18, 96), (36, 96), (64, 16), (96, 33), (128, 16), (16, 161), (0, 16), (16, 0), (72, 96)):
        assert not R.rows_built(Cin, Cout)
        call(MT_ERR_UNSUPPORTED, Cin=Cin, Cout=Cout)
    call(MT_ERR_ARG, amode=1, c1=c1, c2=c2), call(MT_ERR_ARG, amode=1, c0=c0, c2=c2), call(MT_ERR_ARG, amode=1, c0=c0, c1=c1)
    call(MT_ERR_ARG, amode=1, c0=c0, c1=c1, c2=c2, hw=0)
    call(MT_ERR_ARG, amode=2, x2=x2, c1=c1, c2=c2), call(MT_ERR_ARG, amode=2, x2=x2, c0=c0, c2=c2)
    call(MT_ERR_ARG, amode=2, x2=x2, c0=c0, c1=c1), call(MT_ERR_ARG, amode=2, c0=c0, c1=c1, c2=c2)
    call(MT_ERR_ARG, amode=3, c0=c0, c1=c1, c2=c2, x2=x2), call(MT_ERR_ARG, amode=-1)
    call(MT_ERR_ARG, x=_off(x)), call(MT_ERR_ARG, amode=2, x2=_off(x2), c0=c0, c1=c1, c2=c2)
    call(MT_ERR_ARG, amode=1, c0=c0, c1=c1, c2=_off(c2), hw=7)
    r.done(29)


def test_conv1x1_wgrad_refusals():
    r = _Refusals("mt_conv1x1_wgrad")
    du, z, kabc, x, sc, sh, gate = [r.buf(1 << 14) for _ in range(7)]
    dw = r.buf(1 << 14, CANARY, out=True)

    def call(code, du=du, z=z, kabc=kabc, x=x, sc=None, sh=None, gate=None, hw=1, dw=dw, rows=64, Cout=24, Cin=16):
        r.refuse(code, du, z, kabc, x, sc, sh, gate, hw, dw, rows, Cout, Cin)

    for k in ("du", "z", "kabc", "x", "dw"):
        call(MT_ERR_ARG, **{k: None})
    call(MT_ERR_ARG, rows=0), call(MT_ERR_ARG, rows=-1)
    for Cout, Cin in ((18, 16), (16, 18), (96, 96), (160, 96), (96, 160), (288, 16), (16, 288), (260, 64), (0, 16), (16, 0)):
        assert not R.wgrad_supported(Cout, Cin)
        call(MT_ERR_UNSUPPORTED, Cout=Cout, Cin=Cin)
    call(MT_ERR_ARG, gate=gate, sh=sh, hw=7), call(MT_ERR_ARG, gate=gate, sc=sc, hw=7), call(MT_ERR_ARG, gate=gate, sc=sc, sh=sh, hw=0)
    for k, t in (("du", du), ("z", z), ("kabc", kabc), ("x", x)):
        call(MT_ERR_ARG, **{k: _off(t)})
    call(MT_ERR_ARG, gate=_off(gate), sc=sc, sh=sh, hw=7)
    r.done(25)


def test_conv1x1_wgrad_wide_refusals():
    r = _Refusals("mt_conv1x1_wgrad_wide")
    t = {k: r.buf(1 << 16) for k in ("du", "z", "kabc", "x", "sc", "sh", "gate")}
    dw = r.buf(1 << 17, CANARY, out=True)

    def call(code, hw=49, rows=64, Cout=80, Cin=240, **kw):
        a = {**t, "dw": dw, **kw}
        r.refuse(code, a["du"], a["z"], a["kabc"], a["x"], a["sc"], a["sh"], a["gate"], hw, a["dw"], rows, Cout, Cin)

    for k in list(t) + ["dw"]:
        call(MT_ERR_ARG, **{k: None})
    call(MT_ERR_ARG, hw=31), call(MT_ERR_ARG, hw=0), call(MT_ERR_ARG, rows=0), call(MT_ERR_ARG, rows=-32)
    for Cout, Cin in ((64, 240), (324, 240), (80, 220), (80, 2052), (82, 240), (80, 242), (132, 240), (224, 240), (260, 240)):
        assert not R.wide_supported(Cout, Cin)
        call(MT_ERR_UNSUPPORTED, Cout=Cout, Cin=Cin)
    for k in t:
        call(MT_ERR_ARG, **{k: _off(t[k])})
    r.done(28)


def test_conv1x1_bwd_fused_refusals():
    r = _Refusals("mt_conv1x1_bwd_fused")
    t = {k: r.buf(1 << 14) for k in ("du", "kabc", "x", "w", "res")}
    t["dx"], t["dw"] = r.buf(1 << 14, NAN, out=True), r.buf(1 << 14, CANARY, out=True)

    def call(code, rows=64, Cout=96, Cin=16, **kw):
        a = {**t, **kw}
        r.refuse(code, a["du"], a["kabc"], a["x"], a["w"], a["res"], a["dx"], a["dw"], rows, Cout, Cin)

    for k in ("du", "kabc", "x", "w", "dx", "dw"):
        call(MT_ERR_ARG, **{k: None})
    call(MT_ERR_ARG, rows=0), call(MT_ERR_ARG, rows=-64)
    for Cout, Cin in ((96, 36), (96, 0), (96, 18), (128, 16), (64, 16), (92, 16), (140, 16), (148, 16), (160, 16), (144, 36)):
        assert not R.fused_supported(Cout, Cin)
        call(MT_ERR_UNSUPPORTED, Cout=Cout, Cin=Cin)
    for k in ("du", "x", "kabc", "res", "dx"):
        call(MT_ERR_ARG, **{k: _off(t[k])})
    r.done(23)


def test_se_stage_fused_refusals():
    r = _Refusals("mt_se_stage_fused")
    t = {k: r.buf(1 << 15) for k in ("du_p", "z_p", "kabc_p", "w_p", "z_d", "scale_d", "shift_d", "gate", "dpooled", "mi")}
    t["dgate"], t["du_d"] = r.buf(1 << 12, CANARY, out=True), r.buf(1 << 15, NAN, out=True)
    t["stats"] = r.buf(1 << 12, 0.0, F64, out=True)

    def call(code, mode=1, slots=8, rows=128, Co=16, C=96, hw=64, **kw):
        a = {**t, **kw}
        r.refuse(code, a["du_p"], a["z_p"], a["kabc_p"], a["w_p"], a["z_d"], a["scale_d"], a["shift_d"], mode, a["dgate"], a["gate"],
                 a["dpooled"], a["mi"], a["du_d"], a["stats"], slots, rows, Co, C, hw)

    for k in ("du_p", "z_p", "kabc_p", "w_p", "z_d", "scale_d", "shift_d"):
        call(MT_ERR_ARG, **{k: None}), call(MT_ERR_ARG, mode=0, **{k: None})
    for Co, C, hw in ((0, 96, 64), (36, 96, 64), (18, 96, 64), (16, 64, 64), (16, 128, 64), (16, 92, 64), (16, 148, 64), (16, 96, 0),
                      (16, 96, 63), (16, 96, 32), (16, 96, 96)):
        assert not R.se_supported(Co, C, hw)
        call(MT_ERR_UNSUPPORTED, Co=Co, C=C, hw=hw, rows=max(hw, 1) * 2)
    call(MT_ERR_ARG, mode=0, dgate=None)
    for k in ("gate", "dpooled", "mi", "du_d", "stats"):
        call(MT_ERR_ARG, **{k: None})
    call(MT_ERR_ARG, slots=0), call(MT_ERR_ARG, mode=2), call(MT_ERR_ARG, mode=-1)
    call(MT_ERR_ARG, rows=100), call(MT_ERR_ARG, rows=0), call(MT_ERR_ARG, rows=-64), call(MT_ERR_ARG, mode=0, rows=0)
    for k in ("du_p", "z_p", "kabc_p", "z_d", "scale_d", "shift_d"):
        call(MT_ERR_ARG, **{k: _off(t[k])}), call(MT_ERR_ARG, mode=0, **{k: _off(t[k])})
    for k in ("gate", "dpooled", "mi", "du_d"):
        call(MT_ERR_ARG, **{k: _off(t[k])})
    r.done(54)
