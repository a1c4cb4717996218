"""Per-kernel parity of the 3-D convolution (csrc/conv3d.hip: mt_conv3d_fwd with its BatchNorm sums, mt_conv3d_dgrad, mt_conv3d_wgrad
and its splits) against tests/conv3d_ref.py in fp64 on the CPU -- the header's definitions, tied to torch.nn.functional.conv3d and its
autograd by tests/test_conv3d_ref_host.py, which also proves that every case below reaches the branch it was chosen for.  The
conventions are those of tests/test_gpu_train_ends_ops.py and tests/test_gpu_effnet_ops.py: the C ABI is called directly on operands
packed by the reference module, never by the engine; every output (y, dx, dw, ws, part, stats) lies between guard bands of -0.0 in a
buffer of exactly the documented size (a pitched one ends with its last row's last column); written outputs start as NaN, accumulated
ones at known values that the reference adds; the gap columns of a pitched input hold NaN, so that any read of them poisons the
result, and those of a pitched output a canary that must keep its bits.  Figures are per SECTION: y and dx by border rows (some tap
outside the volume or off the output grid) and interior rows, dw by tap, the sum and the sum of squares apart.  A section whose fp64
reference is identically zero -- output rows that read only padding, input rows that no tap reads, taps that never meet the volume --
must be exactly zero (or, accumulated, exactly what was there).  The exact checks (zeros, canaries, guard bands, bit-equality of
repeated and of differently pitched launches, refusals) carry no tolerance; every other gate is twice the worst figure measured on an
MI355X for its kind, rounded up to one significant digit, with that figure, its case and the fp32 yardstick of that case beside it.
MT_TEST_YARDSTICK=1 prints the yardstick (the same reference evaluated in fp32 torch on the CPU against fp64; never gated)."""
import ctypes as C
import functools

import pytest
import torch

from mintime_amd import lib as L

from . import conv3d_ref as R
from .test_gpu_train_ends_ops import _bands_intact, _guarded, _sync_rc
from .test_gpu_tsf_ops import CANARY, MT_ERR_ARG, MT_ERR_UNSUPPORTED, YARD, _d, _Figures
from .util import GRAD_TOL_UNIT, rel_err

pytestmark = pytest.mark.gpu

# gate = 2 x the worst figure measured on an MI355X over every comparison of its kind, one significant digit up.  Beside it: that
# figure and its case, and the yardstick of the same section of the same case.
# Sections have smaller denominators than whole tensors, so the figures lie above the whole-tensor worst case of
# tests/test_gpu_slowfast.py (9.2e-7 at most, here 1.3e-6).  The largest kernel / yardstick ratio over all 548 figures is 3.8
# (fwd.y, r65_c132_k4 plain, interior rows: 4.7e-7 against 1.2e-7).
TOL = {
    "fwd.y": 2e-6,        # 5.9e-7 (asym with the prologue, packed, border rows); yardstick 1.6e-7
    "fwd.sum": 7e-7,      # 3.3e-7 (asym without the prologue, packed); yardstick 1.2e-7
    "fwd.sumsq": 5e-7,    # 2.2e-7 (r65_c132_k4 without the prologue, packed); yardstick 1.2e-7
    "dgrad.dx": 2e-6,     # 5.3e-7 (r129_c132_k132, packed, interior rows); yardstick 5.9e-7
    "wgrad.dw": 3e-6,     # 1.3e-6 (split_r504_asym, splits 1, without the prologue, tap 12 of 30); yardstick 1.4e-6
}
# no gate looser than what the project already accepts for the same kind of quantity
_CEILING = {"y": 2e-5, "dx": 2e-5, "sum": 1e-4, "sumsq": 1e-4, "dw": GRAD_TOL_UNIT}
assert all(v <= _CEILING[k.split(".")[-1]] for k, v in TOL.items())

CANARY_BITS = torch.tensor(CANARY).view(torch.int32).item()
PITCHES = [(0, 0), (4, 8), (12, 8)]          # (ldx - C, ldy - K): packed, and the two pitched forms
_IDS = [c[0] for c in R.CASES]


class _Sections(_Figures):
    """_Figures with the gate looked up by kind, and the rule for sections whose reference is identically zero."""

    def value(self, kind, name, e):
        print(f"FIG {self.what} | {kind} | {name} | {e:.3e} | tol {TOL[kind]:.0e}")
        if not e <= TOL[kind]:
            self.bad.append(f"{kind} {name}: {e:.3e} > {TOL[kind]:.0e}")

    def yard_value(self, kind, name, e):
        print(f"YARD {self.what} | {kind} | {name} | {e:.3e}")

    def rows(self, kind, tag, got, ref, masks, base=None, y32=None):
        """got against ref ([rows, width]) over each row mask apart.  base: what an accumulated output held before."""
        got = got.detach().cpu()
        for name, m in masks.items():
            if not bool(m.any()):
                continue
            if not bool((ref[m] != 0).any()):
                was = torch.zeros_like(got[m]) if base is None else base[m]
                self.true(f"{kind} {tag} {name} rows are exactly {'zero' if base is None else 'what they were'}", torch.equal(got[m] + 0.0, was + 0.0))
                continue
            want = ref[m] if base is None else ref[m] + base[m].double()
            self.value(kind, f"{tag} {name}", rel_err(got[m], want))
            if y32 is not None:
                self.yard_value(kind, f"{tag} {name}", rel_err(y32[m], ref[m]))

    def taps(self, tag, got, ref, g, y32=None):
        """dw [K, taps * C] tap by tap: the worst tap is gated (so every tap is), the taps whose reference is zero are exact."""
        got3, ref3 = got.detach().cpu().double().reshape(g.K, g.taps, g.C), ref.reshape(g.K, g.taps, g.C)
        den, err = ref3.abs().amax((0, 2)), (got3 - ref3).abs().amax((0, 2))
        zero = den == 0
        if bool(zero.any()):
            self.true(f"wgrad.dw {tag}: the {int(zero.sum())} taps that never meet the volume are exactly zero", bool((got3[:, zero] == 0).all()))
        e = torch.where(zero, torch.zeros_like(err), err / den.clamp_min(1e-300))
        worst = int(torch.nan_to_num(e, nan=float("inf")).argmax())
        self.value("wgrad.dw", f"{tag} worst tap ({worst} of {g.taps})", float(e[worst]))
        self.value("wgrad.dw", f"{tag} whole", rel_err(got, ref))
        if y32 is not None:
            e32 = (y32.double().reshape(g.K, g.taps, g.C)[:, worst] - ref3[:, worst]).abs().max() / den[worst].clamp_min(1e-300)
            self.yard_value("wgrad.dw", f"{tag} worst tap ({worst} of {g.taps})", float(e32))
            self.yard_value("wgrad.dw", f"{tag} whole", rel_err(y32, ref))


def _desc(g, ldx=None, ldy=None, **over):
    To, Ho, Wo = g.out
    f = dict(N=g.N, T=g.T, H=g.H, W=g.W, C=g.C, To=To, Ho=Ho, Wo=Wo, K=g.K, kt=g.k[0], kh=g.k[1], kw=g.k[2], st=g.s[0], sh=g.s[1],
             sw=g.s[2], pt=g.p[0], ph=g.p[1], pw=g.p[2], ldx=ldx or g.C, ldy=ldy or g.K)
    f.update(over)
    return L.Conv3dDesc(**f)


def _operand(t5, ld):
    """A [N, C, T, H, W] host tensor as device rows at pitch ld, the gap columns NaN: exactly (rows - 1) ld + C floats."""
    r = R.rows(t5, ld)
    return _d(r.reshape(-1)[:(r.shape[0] - 1) * ld + t5.shape[1]])


class _Out:
    """An output of `n` rows of `width` floats at pitch ld in a guarded buffer of exactly (n - 1) ld + width floats: the data columns
    NaN (a written output) or `base` (an accumulated one), the gap columns the canary."""

    def __init__(self, n, width, ld, base=None):
        self.n, self.width, self.ld = n, width, ld
        host = torch.full((n, ld), CANARY)
        host[:, :width] = float("nan") if base is None else base
        self.numel = (n - 1) * ld + width
        self.buf, self.body = _guarded(self.numel)
        self.body.copy_(_d(host.reshape(-1)[:self.numel]))

    def _wide(self):
        return torch.cat([self.body, self.body.new_full((self.n * self.ld - self.numel,), CANARY)]).reshape(self.n, self.ld)

    def data(self):
        return self._wide()[:, :self.width].contiguous()

    def intact(self):
        """The guard bands and every gap column keep their bits."""
        gaps = self._wide()[:, self.width:].contiguous().view(torch.int32)
        return _bands_intact(self.buf) and bool((gaps == CANARY_BITS).all())


@functools.lru_cache(maxsize=None)
def _case(case):
    """Operands (host fp32, in torch layout and packed) and the fp64 references of one table entry, computed once and shared by the
    tests; read-only.  With MT_TEST_YARDSTICK the same references in fp32 as well."""
    g = R.geo(case)
    x, w, dy, scale, shift = R.inputs(case)
    c = dict(g=g, x=x, dy=dy, wp=R.pack_w(w, g.C), wt=R.pack_wt(w), scale=scale, shift=shift)
    for dt, key in ((torch.float64, "ref"),) + (((torch.float32, "yard"),) if YARD else ()):
        xr, dyr, wp, wt, sc, sh = (t.to(dt) for t in (R.rows(x), R.rows(dy), c["wp"], c["wt"], scale, shift))
        out = {"dx": R.dgrad_ref(g, dyr, wt)}
        for pro, (a, b) in ((False, (None, None)), (True, (sc, sh))):
            y = R.fwd_ref(g, xr, wp, a, b)
            out["y", pro], out["stats", pro], out["dw", pro] = y, R.stats_ref(y), R.wgrad_ref(g, xr, dyr, a, b)
        c[key] = out
    c["dev"] = {k: _d(c[k]) for k in ("wp", "wt", "scale", "shift")}
    c["ysec"], c["xsec"] = R.y_sections(g), R.dx_sections(g)
    return c


def _base(n, width, seed):
    return torch.randn(n, width, generator=torch.Generator().manual_seed(seed))


def _fwd(c, pro, ldx, ldy, base=None, stats=True):
    g, dv, lib = c["g"], c["dev"], L.get()
    d = _desc(g, ldx, ldy)
    x = _operand(c["x"], ldx)
    y = _Out(g.rows_out, g.K, ldy, base)
    pbuf = part = sbuf = st = None
    if stats:
        pbuf, part = _guarded(int(lib.mt_conv3d_part_floats(C.byref(d))))
        sbuf, st = _guarded(2 * g.K, dtype=torch.float64)
    L.check(lib.mt_conv3d_fwd(C.byref(d), L.ptr(x), L.ptr(dv["scale"] if pro else None), L.ptr(dv["shift"] if pro else None),
                              L.ptr(dv["wp"]), L.ptr(y.body), int(base is not None), L.ptr(part), L.ptr(st), L.stream_ptr()), "mt_conv3d_fwd")
    torch.cuda.synchronize()
    ok = y.intact() and (not stats or (_bands_intact(pbuf) and _bands_intact(sbuf)))
    return y.data(), (st.reshape(2, g.K).cpu() if stats else None), ok


def _dgrad(c, ldx, ldy, base=None):
    g = c["g"]
    d = _desc(g, ldx, ldy)
    dy = _operand(c["dy"], ldy)
    dx = _Out(g.rows_in, g.C, ldx, base)
    L.check(L.get().mt_conv3d_dgrad(C.byref(d), L.ptr(dy), L.ptr(c["dev"]["wt"]), L.ptr(dx.body), int(base is not None), L.stream_ptr()),
            "mt_conv3d_dgrad")
    torch.cuda.synchronize()
    return dx.data(), dx.intact()


def _wgrad(c, pro, ldx, ldy, splits=None):
    """splits None: the planner's own count.  ws holds exactly splits * K * taps * C floats (none for one split)."""
    g, dv, lib = c["g"], c["dev"], L.get()
    d = _desc(g, ldx, ldy)
    if splits is None:
        splits = int(lib.mt_conv3d_wgrad_splits(C.byref(d)))
    x, dy = _operand(c["x"], ldx), _operand(c["dy"], ldy)
    n = g.K * g.taps * g.C
    dbuf, dw = _guarded(n)
    wbuf, ws = _guarded(splits * n) if splits > 1 else (None, None)
    L.check(lib.mt_conv3d_wgrad(C.byref(d), L.ptr(x), L.ptr(dv["scale"] if pro else None), L.ptr(dv["shift"] if pro else None), L.ptr(dy),
                                L.ptr(dw), L.ptr(ws), splits, L.stream_ptr()), "mt_conv3d_wgrad")
    torch.cuda.synchronize()
    return dw.reshape(g.K, -1), _bands_intact(dbuf) and (wbuf is None or _bands_intact(wbuf))


def _pitch_tag(dx, dy):
    return "packed" if not dx and not dy else f"ldx C+{dx} ldy K+{dy}"


# ---- 1. forward -----------------------------------------------------------------------------------------------------------------------

def _check_stats(fig, tag, st, ref, y32=None):
    fig.true(f"{tag}: every sum is written", bool(torch.isfinite(st).all()))
    fig.value("fwd.sum", f"{tag} sum", rel_err(st[0], ref[0]))
    fig.value("fwd.sumsq", f"{tag} sum of squares", rel_err(st[1], ref[1]))
    if y32 is not None:
        fig.yard_value("fwd.sum", f"{tag} sum", rel_err(y32[0], ref[0]))
        fig.yard_value("fwd.sumsq", f"{tag} sum of squares", rel_err(y32[1], ref[1]))


@pytest.mark.parametrize("pro", [False, True], ids=["plain", "pro"])
@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_forward_vs_fp64(case, pro):
    """mt_conv3d_fwd: y by border and interior rows, the two BatchNorm sums apart, rows that read only padding exactly zero; packed with
    statistics (twice: the same bits), pitched by (C + 4, K + 8) accumulating onto known values, pitched by (C + 12, K + 8) with
    statistics (the same y and statistics bits as packed)."""
    c = _case(case)
    g, ref = c["g"], c["ref"]
    yard = c.get("yard")
    fig = _Sections(f"fwd {case[0]} {'pro' if pro else 'plain'}")
    y0, st0, ok = _fwd(c, pro, g.C, g.K)
    fig.true("packed: nothing written outside y, part and stats", ok)
    fig.rows("fwd.y", "packed", y0, ref["y", pro], c["ysec"], y32=yard and yard["y", pro])
    _check_stats(fig, "packed", st0, ref["stats", pro], yard and yard["stats", pro])
    y1, st1, ok = _fwd(c, pro, g.C, g.K)
    fig.true("second launch: the same y and statistics bits", ok and torch.equal(y1, y0) and torch.equal(st1, st0))
    base = _base(g.rows_out, g.K, 7)
    ya, _, ok = _fwd(c, pro, g.C + 4, g.K + 8, base=base, stats=False)
    fig.true("accumulate, pitched: guard bands and gap columns keep their bits", ok)
    fig.rows("fwd.y", "accumulate ldx C+4 ldy K+8", ya, ref["y", pro], c["ysec"], base=base)
    y2, st2, ok = _fwd(c, pro, g.C + 12, g.K + 8)
    fig.true("ldx C+12 ldy K+8: guard bands and gap columns keep their bits", ok)
    fig.true("ldx C+12 ldy K+8: the same y and statistics bits as packed", torch.equal(y2, y0) and torch.equal(st2, st0))
    y3, _, ok = _fwd(c, pro, g.C, g.K, stats=False)
    fig.true("part = stats = NULL: the same y bits", ok and torch.equal(y3, y0))
    fig.done()


def test_forward_statistics_two_level_reduction():
    """32769 rows = 513 blocks of 64: the statistics' partial rows exceed one chunk of 512, so the sums go through the second level,
    whose last chunk holds one row; part is guarded at exactly mt_conv3d_part_floats(d)."""
    c = _case(R.BIG_CASE)
    g, ref = c["g"], c["ref"]
    yard = c.get("yard")
    assert -(-g.rows_out // R.BM) == 513
    fig = _Sections(f"fwd {R.BIG_CASE[0]} pro")
    y, st, ok = _fwd(c, True, g.C, g.K)
    fig.true("nothing written outside y, part and stats", ok)
    fig.rows("fwd.y", "packed", y, ref["y", True], c["ysec"], y32=yard and yard["y", True])
    tail = {"the last block's one row": torch.arange(g.rows_out) == g.rows_out - 1}
    fig.rows("fwd.y", "packed", y, ref["y", True], tail)
    _check_stats(fig, "packed", st, ref["stats", True], yard and yard["stats", True])
    _, st1, ok = _fwd(c, True, g.C, g.K)
    fig.true("second launch: the same statistics bits", ok and torch.equal(st1, st))
    fig.done()


# ---- 2. data gradient -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_data_gradient_vs_fp64(case):
    """mt_conv3d_dgrad: dx by border and interior rows, the rows no tap reads exactly zero (accumulated: exactly what they were);
    packed (twice: the same bits), then dy pitched by K + 8 (NaN gaps) with dx pitched by C + 4 accumulating and by C + 12 written."""
    c = _case(case)
    g, ref = c["g"], c["ref"]["dx"]
    yard = c.get("yard")
    fig = _Sections(f"dgrad {case[0]}")
    d0, ok = _dgrad(c, g.C, g.K)
    fig.true("packed: nothing written outside dx", ok)
    fig.rows("dgrad.dx", "packed", d0, ref, c["xsec"], y32=yard and yard["dx"])
    d1, ok = _dgrad(c, g.C, g.K)
    fig.true("second launch: the same bits", ok and torch.equal(d1, d0))
    base = _base(g.rows_in, g.C, 11)
    da, ok = _dgrad(c, g.C + 4, g.K + 8, base=base)
    fig.true("accumulate, pitched: guard bands and gap columns keep their bits", ok)
    fig.rows("dgrad.dx", "accumulate ldx C+4 ldy K+8", da, ref, c["xsec"], base=base)
    d2, ok = _dgrad(c, g.C + 12, g.K + 8)
    fig.true("ldx C+12 ldy K+8: guard bands and gap columns keep their bits, the same bits as packed", ok and torch.equal(d2, d0))
    fig.done()


# ---- 3. weight gradient ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pro", [False, True], ids=["plain", "pro"])
@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_weight_gradient_vs_fp64(case, pro):
    """mt_conv3d_wgrad at the planner's split count: dw tap by tap, the taps that never meet the volume exactly zero; x and dy packed
    (twice: the same bits) and pitched with NaN in their gap columns (the same bits as packed)."""
    c = _case(case)
    g, ref = c["g"], c["ref"]["dw", pro]
    yard = c.get("yard")
    fig = _Sections(f"wgrad {case[0]} {'pro' if pro else 'plain'}")
    w0 = None
    for dx, dy in PITCHES + [(0, 0)]:
        dw, ok = _wgrad(c, pro, g.C + dx, g.K + dy)
        tag = _pitch_tag(dx, dy)
        fig.true(f"{tag}: nothing written outside dw and ws", ok)
        if w0 is None:
            w0 = dw
            fig.taps(tag, dw, ref, g, yard and yard["dw", pro])
        else:
            fig.true(f"{tag}: the same bits as the first packed launch", torch.equal(dw, w0))
    fig.done()


@pytest.mark.parametrize("kernel", list(R.SPLIT_KERNELS))
@pytest.mark.parametrize("rows", list(R.SPLIT_GRIDS))
def test_weight_gradient_splits_vs_fp64(rows, kernel):
    """Every split count of the table, and the planner's own, over `rows` output rows: each meets the gate tap by tap (different counts
    may differ in their bits), dw and a ws of exactly splits * K * taps * C floats stay inside their guard bands, and a second launch
    with the same count gives the same bits."""
    case = R.split_case(rows, kernel)
    c = _case(case)
    g, lib = c["g"], L.get()
    own = int(lib.mt_conv3d_wgrad_splits(C.byref(_desc(g))))
    fig = _Sections(f"wgrad {case[0]}")
    for splits in R.split_counts(rows) + [own]:
        for pro in (False, True):
            tag = f"splits {splits}{' (planner)' if splits == own else ''} {'pro' if pro else 'plain'}"
            dw, ok = _wgrad(c, pro, g.C, g.K, splits)
            fig.true(f"{tag}: nothing written outside dw and ws", ok)
            fig.taps(tag, dw, c["ref"]["dw", pro], g, c.get("yard") and c["yard"]["dw", pro])
            dw2, ok = _wgrad(c, pro, g.C, g.K, splits)
            fig.true(f"{tag}: second launch, the same bits", ok and torch.equal(dw2, dw))
    fig.done()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    """Everything refused here is refused on the host: check_desc and each entry point's pointer, pairing, split-count and alignment
    checks all return before the first launch (csrc/conv3d.hip).  The documented code comes back, mt_last_error names the reason, and
    every output keeps its canary.  (Statistics of an accumulated output: tests/test_gpu_slowfast_ops.py.)"""
    lib, st = L.get(), L.stream_ptr()
    g = R.geo(R.ASYM_CASES[0])
    n = g.K * g.taps * g.C
    x, dy, wp, wt, sc, sh = (torch.ones(k + 4, device="cuda") for k in (g.rows_in * g.C, g.rows_out * g.K, n, n, g.C, g.C))
    sizes = dict(y=g.rows_out * g.K, dx=g.rows_in * g.C, dw=n, ws=2 * n, part=int(lib.mt_conv3d_part_floats(C.byref(_desc(g)))))
    o = {k: _guarded(v, CANARY) for k, v in sizes.items()}
    o["stats"] = _guarded(2 * g.K, CANARY, torch.float64)
    b = {k: v[1] for k, v in o.items()}
    fig = _Figures("conv3d refusals")

    def ref(d):
        return None if d is None else C.byref(d)

    def fwd(d, x_=x, w_=wp, y_=b["y"], sc_=None, sh_=None, part=None, stats=None):
        return lib.mt_conv3d_fwd(ref(d), L.ptr(x_), L.ptr(sc_), L.ptr(sh_), L.ptr(w_), L.ptr(y_), 0, L.ptr(part), L.ptr(stats), st)

    def dgrad(d, dy_=dy, wt_=wt, dx_=b["dx"]):
        return lib.mt_conv3d_dgrad(ref(d), L.ptr(dy_), L.ptr(wt_), L.ptr(dx_), 0, st)

    def wgrad(d, x_=x, dy_=dy, dw_=b["dw"], ws_=b["ws"], splits=2, sc_=None, sh_=None):
        return lib.mt_conv3d_wgrad(ref(d), L.ptr(x_), L.ptr(sc_), L.ptr(sh_), L.ptr(dy_), L.ptr(dw_), L.ptr(ws_), splits, st)

    def refused(what, rc, code, fragment):
        msg = (lib.mt_last_error() or b"").decode()
        fig.true(f"{what}: code {code} and '{fragment}' (got {_sync_rc(rc)}: {msg})", rc == code and fragment in msg)

    good = _desc(g)
    bad_desc = [("null descriptor", None, MT_ERR_ARG, "null descriptor"),
                ("N = 0", _desc(g, N=0), MT_ERR_ARG, "empty or negative shape"),
                ("kw = 0", _desc(g, kw=0), MT_ERR_ARG, "empty or negative shape"),
                ("sh = 0", _desc(g, sh=0), MT_ERR_ARG, "empty or negative shape"),
                ("K = -4", _desc(g, K=-4), MT_ERR_ARG, "empty or negative shape"),
                ("pt = -1", _desc(g, pt=-1), MT_ERR_ARG, "empty or negative shape"),
                ("To + 1", _desc(g, To=g.out[0] + 1), MT_ERR_ARG, "does not match"),
                ("Ho - 1", _desc(g, Ho=g.out[1] - 1), MT_ERR_ARG, "does not match"),
                ("Wo + 1", _desc(g, Wo=g.out[2] + 1), MT_ERR_ARG, "does not match"),
                ("C % 4", _desc(g, C=g.C - 2), MT_ERR_UNSUPPORTED, "multiples of 4"),
                ("K % 4", _desc(g, K=g.K - 2), MT_ERR_UNSUPPORTED, "multiples of 4"),
                ("ldx % 4", _desc(g, ldx=g.C + 2), MT_ERR_UNSUPPORTED, "multiples of 4"),
                ("ldy % 4", _desc(g, ldy=g.K + 2), MT_ERR_UNSUPPORTED, "multiples of 4"),
                ("ldx < C", _desc(g, ldx=g.C - 4), MT_ERR_UNSUPPORTED, "pitches >= widths"),
                ("ldy < K", _desc(g, ldy=g.K - 4), MT_ERR_UNSUPPORTED, "pitches >= widths")]
    for name, call in (("mt_conv3d_fwd", fwd), ("mt_conv3d_dgrad", dgrad), ("mt_conv3d_wgrad", wgrad)):
        for what, d, code, fragment in bad_desc:
            refused(f"{name}, {what}", call(d), code, fragment)
            fig.true(f"{name}, {what}: the message names the entry point", (lib.mt_last_error() or b"").decode().startswith(name))

    for k in ("x_", "w_", "y_"):
        refused(f"fwd, {k} NULL", fwd(good, **{k: None}), MT_ERR_ARG, "mt_conv3d_fwd: null pointer")
    refused("fwd, scale without shift", fwd(good, sc_=sc), MT_ERR_ARG, "scale and shift go together")
    refused("fwd, shift without scale", fwd(good, sh_=sh), MT_ERR_ARG, "scale and shift go together")
    refused("fwd, part without stats", fwd(good, part=b["part"]), MT_ERR_ARG, "part and stats go together")
    refused("fwd, stats without part", fwd(good, stats=b["stats"]), MT_ERR_ARG, "part and stats go together")
    refused("fwd, x off a 16-byte boundary", fwd(good, x_=x[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")
    refused("fwd, w off a 16-byte boundary", fwd(good, w_=wp[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")
    refused("fwd, scale off a 16-byte boundary", fwd(good, sc_=sc[1:], sh_=sh), MT_ERR_UNSUPPORTED, "16-byte aligned")
    refused("fwd, shift off a 16-byte boundary", fwd(good, sc_=sc, sh_=sh[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")

    for k in ("dy_", "wt_", "dx_"):
        refused(f"dgrad, {k} NULL", dgrad(good, **{k: None}), MT_ERR_ARG, "mt_conv3d_dgrad: null pointer")
    refused("dgrad, dy off a 16-byte boundary", dgrad(good, dy_=dy[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")
    refused("dgrad, wt off a 16-byte boundary", dgrad(good, wt_=wt[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")

    for k in ("x_", "dy_", "dw_"):
        refused(f"wgrad, {k} NULL", wgrad(good, **{k: None}), MT_ERR_ARG, "null pointer or bad split count")
    refused("wgrad, splits 0", wgrad(good, splits=0), MT_ERR_ARG, "null pointer or bad split count")
    refused("wgrad, splits -1", wgrad(good, splits=-1), MT_ERR_ARG, "null pointer or bad split count")
    refused("wgrad, splits 2 without ws", wgrad(good, ws_=None), MT_ERR_ARG, "null pointer or bad split count")
    refused("wgrad, scale without shift", wgrad(good, sc_=sc), MT_ERR_ARG, "scale and shift go together")
    refused("wgrad, x off a 16-byte boundary", wgrad(good, x_=x[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")
    refused("wgrad, dy off a 16-byte boundary", wgrad(good, dy_=dy[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")
    refused("wgrad, shift off a 16-byte boundary", wgrad(good, sc_=sc, sh_=sh[1:]), MT_ERR_UNSUPPORTED, "16-byte aligned")

    torch.cuda.synchronize()
    fig.true("every output keeps its canary", all(bool((body == CANARY).all()) and _bands_intact(buf) for buf, body in o.values()))
    fig.done()
