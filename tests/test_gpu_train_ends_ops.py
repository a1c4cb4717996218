"""Per-kernel parity of the kernels at the two ends of a training step -- the Baseline head (csrc/baseline.hip), BCE-with-logits and the
multi-tensor SGD / Adam (csrc/optim.hip), the dropout passes (csrc/dropout.hip) and the fixed-order BatchNorm sums (mt_det_bn_sums,
csrc/det.hip) -- against plain fp64 torch on the CPU (tests/train_ends_ref.py: the operations' definitions and autograd of them; its
case tables are proven to hold every edge by tests/test_train_ends_ref_host.py).  Same scaffolding as tests/test_gpu_tsf_ops.py: the C
ABI directly, outputs pre-filled with NaN or a canary between guard bands of -0.0 checked by bit pattern, shapes picked for the kernels'
tails and dispatch thresholds, comparison per section.  The exact checks (guards, canaries, refusals, bit-equalities, signs) have no
tolerance; every other gate is twice the worst case measured on an MI355X against the fp64 reference, rounded up to one significant
digit, with that worst case, its case and the yardstick (the same reference evaluated in fp32 torch on the CPU, against fp64) next to
it.  MT_TEST_YARDSTICK=1 prints the yardstick figures beside the kernels'."""
import functools

import pytest
import torch

from mintime_amd import lib as L

from . import train_ends_ref as R
from .test_gpu_tsf_ops import CANARY, MT_ERR_ARG, MT_ERR_UNSUPPORTED, YARD, _d, _Figures, dev
from .util import GRAD_TOL_UNIT

pytestmark = pytest.mark.gpu

# gate = 2 x the worst case measured on an MI355X over every comparison that uses it, one significant digit up.  Beside it: that worst
# case, and the yardstick -- the largest error of the same reference evaluated in fp32 torch on the CPU against fp64, same cases.
HEAD_FWD_TOL = {"moderate": 5e-7,          # 2.1e-7 (v, n 2 hw 3 C 1280 m 512, NHWC); yardstick 6.4e-7
                "offset": 1e-5}            # 4.9e-6 (logits, n 2 hw 3 C 1280 m 512, NCHW); yardstick 2.2e-5: 1280 products of ~1e3 v[c]
#                                            of both signs cancel in the logit
HEAD_BWD_TOL = {"moderate": 5e-7,          # 2.1e-7 (dW1, n 33 hw 64 C 256 m 5, NCHW); yardstick 8.0e-7
                "offset": 6e-6}            # 2.8e-6 (dW1, n 65 hw 9 C 508 m 16, NHWC); yardstick 3.6e-6: u = sum_i g_i pooled_i with
#                                            pooled ~ 1e3 and g of both signs cancels to ~1e-2 of its terms
BCE_TOL = {"moderate": 3e-7,               # 1.4e-7 (n dx, n 1000, hard labels, pos_weight 1); yardstick 1.4e-7
           "saturated": 2e-7,              # 9.1e-8 (loss, n 1000, soft labels, pos_weight 0.4); yardstick 9.4e-8
           "tiny": 3e-7}                   # 1.5e-7 (n dx, n 1000, hard labels, pos_weight 1); yardstick 2.1e-7
SGD_TOL = 2e-7                             # 5.6e-8 (the aligned 8193-element tensor, wd 1e-2); yardstick 5.5e-8
ADAM_TOL = 3e-7                            # 1.2e-7 (v at gradient scale 1e6, Adam, wd 0, t 1); yardstick 1.2e-7
MUL_ADD_TOL = 1e-7                         # 5.0e-8 (n 8388612); yardstick 7.1e-8
GEGLU_TOL = {"moderate": 9e-7,             # 4.1e-7 (dg, n_half 8, 1 row, m given); yardstick 6.1e-7
             "tails": 3e-7,                # 1.1e-7 (dg, n_half 8, 100 rows, m given); yardstick 1.4e-7
             "tiny": 9e-7}                 # 4.2e-7 (dg, n_half 72, 33 rows, m given); yardstick 4.2e-7
# the BatchNorm sums accumulate in fp64 (the reference's column sums are correctly rounded, math.fsum): these two are fp64 figures
BN_S1_TOL = 2e-16                          # 8.6e-17 (moderate, 1 row, C 32: the one rounding of start + x); yardstick 2.0e-7
BN_S2_TOL = {0: 6e-15,                     # 2.6e-15 (offset, 2049 rows, C 32); yardstick 2.0e-7
             1: 4e-7}                      # 1.5e-7 (moderate, 15 rows, C 1); yardstick 2.6e-7: the kernel forms this product in fp32
assert max(max(HEAD_FWD_TOL.values()), max(HEAD_BWD_TOL.values()), max(BCE_TOL.values()), SGD_TOL, ADAM_TOL, MUL_ADD_TOL,
           max(GEGLU_TOL.values()), BN_S1_TOL, max(BN_S2_TOL.values())) <= GRAD_TOL_UNIT
assert max(HEAD_FWD_TOL["moderate"], BCE_TOL["moderate"], MUL_ADD_TOL, BN_S1_TOL, max(BN_S2_TOL.values())) <= 1e-5


def _guarded(numel, fill=float("nan"), dtype=torch.float32):
    """A device buffer of `numel` elements holding `fill`, between two 64-element guard bands of -0.0 (any store into a band shows,
    and so does a read-modify-write that adds +0.0)."""
    buf = torch.full((numel + 128,), -0.0, dtype=dtype, device=dev)
    body = buf[64:64 + numel]
    body.fill_(fill)
    return buf, body


def _sign_bits(t):
    """The elements of a floating tensor as integers, and the bit pattern of -0.0 in that width."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.view(it), -(1 << (8 * t.element_size() - 1))


def _bands_intact(buf):
    bits, neg0 = _sign_bits(buf)
    return bool((bits[:64] == neg0).all() and (bits[-64:] == neg0).all())


def _sync_rc(rc):
    torch.cuda.synchronize()
    return rc


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. the Baseline head ----------------------------------------------------------------------------------------------------------

_HEAD_IDS = [f"n{n}-hw{hw}-C{C}-m{m}" for n, hw, C, m in R.HEAD_CASES]


@functools.lru_cache(maxsize=None)
def _head_case(case, layout, regime):
    """Inputs (fp32, host and device) and the fp64 references of one head case, computed once and shared by the tests; read-only."""
    n, hw, C, m = case
    host = R.head_inputs(n, hw, C, m, layout, regime, seed=1000 * layout + sum(case))
    x, w1, b1, w2, b2, dl = (t.double() for t in host)
    fwd = R.baseline_head(x, layout, w1, b1, w2, b2)
    bwd = R.baseline_head_bwd(x, layout, w1, b1, w2, b2, dl)
    return host, tuple(_d(t) for t in host), fwd, bwd


def _head_fwd(devs, layout, case, with_pooled=True):
    n, hw, C, m = case
    x, w1, b1, w2, b2, _ = devs
    S = (C + R.HEAD_CHUNK - 1) // R.HEAD_CHUNK
    vbuf, vc = _guarded(C + 1)
    pbuf, pooled = _guarded(n * C) if with_pooled else (None, None)
    tbuf, part = _guarded(n * S)
    lbuf, logits = _guarded(n)
    L.check(L.get().mt_baseline_head_fwd(L.ptr(x), layout, n, hw, C, m, L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(vc), L.ptr(pooled),
                                         L.ptr(part), L.ptr(logits), L.stream_ptr()), "mt_baseline_head_fwd")
    torch.cuda.synchronize()
    ok = all(_bands_intact(b) for b in (vbuf, pbuf, tbuf, lbuf) if b is not None)
    return vc, (pooled.reshape(n, C) if with_pooled else None), part, logits, ok


@pytest.mark.parametrize("regime", R.HEAD_REGIMES)
@pytest.mark.parametrize("layout", R.HEAD_LAYOUTS)
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=_HEAD_IDS)
def test_baseline_head_forward_vs_fp64(case, layout, regime):
    """v, c0, pooled and logits of mt_baseline_head_fwd, each its own section, against AdaptiveAvgPool2d(1) -> Linear -> Linear in fp64;
    vc (C + 1), pooled, part (exactly n * ceil(C / 256)) and logits sit between guard bands; pooled = NULL gives the same logits."""
    n, hw, C, m = case
    host, devs, (logits_ref, pooled_ref, v_ref, c0_ref), _ = _head_case(case, layout, regime)
    fig = _Figures(f"head_fwd {regime} n{n} hw{hw} C{C} m{m} layout{layout}")
    tol = HEAD_FWD_TOL[regime]
    vc, pooled, part, logits, ok = _head_fwd(devs, layout, case)
    fig.true("nothing written outside vc / pooled / part / logits", ok)
    fig.true("every element of vc, pooled, part and logits is written",
             all(bool(torch.isfinite(t).all()) for t in (vc, pooled, part, logits)))
    fig.close("v", vc[:C], v_ref, tol)
    fig.close("c0", vc[C:], c0_ref.reshape(1), tol)
    fig.close("pooled", pooled, pooled_ref, tol)
    fig.close("logits", logits, logits_ref, tol)
    if YARD:
        l32, p32, v32, c32 = R.baseline_head(*host[:1], layout, *host[1:5])
        for name, a, b in (("v", v32, v_ref), ("c0", c32.reshape(1), c0_ref.reshape(1)), ("pooled", p32, pooled_ref), ("logits", l32, logits_ref)):
            fig.yard(name, a, b)
    vc2, _, part2, logits2, ok2 = _head_fwd(devs, layout, case, with_pooled=False)
    fig.true("pooled = NULL: same vc, part and logits bits",
             ok2 and torch.equal(vc2, vc) and torch.equal(part2, part) and torch.equal(logits2, logits))
    fig.done()


_HEAD_OUTS = ("dW1", "db1", "dW2", "db2", "dx")


def _head_bwd(devs, fwd_out, layout, case, want):
    """mt_baseline_head_bwd for the outputs named in `want`; what those do not need is not passed (NULL)."""
    n, hw, C, m = case
    _, w1, b1, w2, _, dl = devs
    vc, pooled = fwd_out
    params = any(k != "dx" for k in want)
    sizes = {"dW1": m * C, "db1": m, "dW2": m, "db2": 1, "dx": n * hw * C}
    bufs = {k: _guarded(sizes[k]) for k in want}
    nslab = (n + R.HEAD_SLAB - 1) // R.HEAD_SLAB
    wbuf, work = _guarded((nslab + 1) * (C + 4)) if params else (None, None)
    out = {k: (bufs[k][1] if k in bufs else None) for k in _HEAD_OUTS}
    L.check(L.get().mt_baseline_head_bwd(L.ptr(dl), L.ptr(pooled if params else None), L.ptr(vc), n, hw, C, m,
                                         L.ptr(w1 if "dW2" in want else None), L.ptr(b1 if "dW2" in want else None),
                                         L.ptr(w2 if params else None), L.ptr(out["dW1"]), L.ptr(out["db1"]), L.ptr(out["dW2"]),
                                         L.ptr(out["db2"]), L.ptr(out["dx"]), layout, L.ptr(work), L.stream_ptr()), "mt_baseline_head_bwd")
    torch.cuda.synchronize()
    ok = all(_bands_intact(b) for b, _ in bufs.values()) and (wbuf is None or _bands_intact(wbuf))
    return {k: bufs[k][1] for k in want}, ok


@pytest.mark.parametrize("regime", R.HEAD_REGIMES)
@pytest.mark.parametrize("layout", R.HEAD_LAYOUTS)
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=_HEAD_IDS)
def test_baseline_head_backward_vs_fp64(case, layout, regime):
    """dW1, db1, dW2, db2 and dx of mt_baseline_head_bwd against autograd of the definition in fp64: all five together (twice:
    bit-identical), then each alone with every other pointer NULL (bit-equal to the joint call); `work` is guarded at exactly
    (ceil(n / 32) + 1)(C + 4) floats; dx is exactly constant over a crop's pixels."""
    n, hw, C, m = case
    host, devs, _, ref = _head_case(case, layout, regime)
    fig = _Figures(f"head_bwd {regime} n{n} hw{hw} C{C} m{m} layout{layout}")
    tol = HEAD_BWD_TOL[regime]
    vc, pooled, _, _, ok = _head_fwd(devs, layout, case)
    fig.true("forward wrote nothing outside its outputs", ok)
    shapes = {"dW1": (m, C), "db1": (m,), "dW2": (m,), "db2": (1,), "dx": ref["dx"].shape}
    joint, ok = _head_bwd(devs, (vc, pooled), layout, case, _HEAD_OUTS)
    fig.true("joint call: nothing written outside the outputs and work", ok)
    for k in _HEAD_OUTS:
        fig.close(k, joint[k].reshape(shapes[k]), ref[k], tol)
    if YARD:
        r32 = R.baseline_head_bwd(host[0], layout, *host[1:])
        for k in _HEAD_OUTS:
            fig.yard(k, r32[k], ref[k])
    dx = joint["dx"].reshape(shapes["dx"])
    first = dx[:, :1, :] if layout == 0 else dx[:, :, :1]
    fig.true("dx is exactly constant over a crop's pixels", (dx == first).all())
    again, ok = _head_bwd(devs, (vc, pooled), layout, case, _HEAD_OUTS)
    fig.true("second launch bit-identical", ok and all(torch.equal(again[k], joint[k]) for k in _HEAD_OUTS))
    for k in _HEAD_OUTS:
        lone, ok = _head_bwd(devs, (vc, pooled), layout, case, (k,))
        fig.true(f"{k} alone: bit-equal to the joint call, nothing written elsewhere", ok and torch.equal(lone[k], joint[k]))
    fig.done()


def test_baseline_head_refusals_write_nothing():
    """Every refusal is decided on the host (check_shape and the pointer checks of the two entry points come before the first launch):
    the documented code comes back and every output keeps its canary.  n = 65536 is refused before any buffer is looked at, so the
    buffers here stay those of the two-crop case."""
    lib = L.get()
    n, hw, C, m = 2, 3, 8, 4
    g = _gen(0)
    x, w1, b1, w2, b2, dl = (_d(torch.randn(s, generator=g)) for s in ((n * hw * C + 4,), (m * C + 4,), (m,), (m,), (1,), (n,)))
    names = ("vc", "pooled", "part", "logits", "dW1", "db1", "dW2", "db2", "dx", "work")
    sizes = (C + 1 + 4, n * C, n, n, m * C + 4, m, m, 1, n * hw * C + 4, 2 * (C + 4) + 4)
    o = {k: _guarded(s, CANARY) for k, s in zip(names, sizes)}
    b = {k: v[1] for k, v in o.items()}
    st = L.stream_ptr()

    def fwd(x_=x, layout=0, n_=n, C_=C, vc=b["vc"]):
        return _sync_rc(lib.mt_baseline_head_fwd(L.ptr(x_), layout, n_, hw, C_, m, L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(vc),
                                                 L.ptr(b["pooled"]), L.ptr(b["part"]), L.ptr(b["logits"]), st))

    def bwd(layout=0, n_=n, C_=C, vc=b["vc"], pooled=b["pooled"], w1_=w1, dw1=b["dW1"], db1=b["db1"], dw2=b["dW2"], db2=b["db2"], dx=b["dx"],
            work=b["work"]):
        return _sync_rc(lib.mt_baseline_head_bwd(L.ptr(dl), L.ptr(pooled), L.ptr(vc), n_, hw, C_, m, L.ptr(w1_), L.ptr(b1), L.ptr(w2), L.ptr(dw1),
                                                 L.ptr(db1), L.ptr(dw2), L.ptr(db2), L.ptr(dx), layout, L.ptr(work), st))

    fig = _Figures("head refusals")
    for call, tag in ((fwd, "fwd"), (bwd, "bwd")):
        fig.true(f"{tag}: C % 4 != 0 is unsupported", call(C_=6) == MT_ERR_UNSUPPORTED)
        fig.true(f"{tag}: layout 2 is an argument error", call(layout=2) == MT_ERR_ARG)
        fig.true(f"{tag}: n = 0 is an argument error", call(n_=0) == MT_ERR_ARG)
        fig.true(f"{tag}: n = 65536 is unsupported", call(n_=65536) == MT_ERR_UNSUPPORTED)
        fig.true(f"{tag}: vc off a 16-byte boundary", call(vc=b["vc"][1:]) == MT_ERR_UNSUPPORTED)
    fig.true("fwd: x off a 16-byte boundary", fwd(x_=x[1:]) == MT_ERR_UNSUPPORTED)
    fig.true("bwd: dx off a 16-byte boundary", bwd(dx=b["dx"][1:]) == MT_ERR_UNSUPPORTED)
    fig.true("bwd: work off a 16-byte boundary", bwd(work=b["work"][1:]) == MT_ERR_UNSUPPORTED)
    fig.true("bwd: dW1 off a 16-byte boundary", bwd(dw1=b["dW1"][1:]) == MT_ERR_UNSUPPORTED)
    fig.true("bwd: W1 off a 16-byte boundary (dW2 asked for)", bwd(w1_=w1[1:]) == MT_ERR_UNSUPPORTED)
    for k in ("dw1", "db1", "dw2", "db2"):
        only = {q: None for q in ("dw1", "db1", "dw2", "db2", "dx") if q != k}
        fig.true(f"bwd: {k} without pooled is an argument error", bwd(pooled=None, **only) == MT_ERR_ARG)
        fig.true(f"bwd: {k} without work is an argument error", bwd(work=None, **only) == MT_ERR_ARG)
    fig.true("every output keeps its canary", all(bool((body == CANARY).all()) and _bands_intact(buf) for buf, body in o.values()))
    fig.done()


# ---- 2. BCE with logits --------------------------------------------------------------------------------------------------------------

def _bce(x_d, y_d, pw, n, with_dx=True):
    lbuf, loss = _guarded(1)
    dbuf, dx = _guarded(n) if with_dx else (None, None)
    L.check(L.get().mt_bce_logits(L.ptr(x_d), L.ptr(y_d), pw, L.ptr(loss), L.ptr(dx), n, L.stream_ptr()), "mt_bce_logits")
    torch.cuda.synchronize()
    return loss, dx, _bands_intact(lbuf) and (dbuf is None or _bands_intact(dbuf))


@pytest.mark.parametrize("regime", R.BCE_REGIMES)
@pytest.mark.parametrize("n", R.BCE_N)
def test_bce_logits_vs_fp64(n, regime):
    """loss and n * dloss/dx of mt_bce_logits against autograd of binary_cross_entropy_with_logits in fp64, for every pos_weight and
    hard and soft (0.3) labels; `saturated` draws the logits from +-{30, 88, 89, 104, 230}, either side of expf overflow and of
    flush-to-zero: everything stays finite, and the gradient keeps its sign where the label is 0 or 1."""
    fig = _Figures(f"bce {regime} n{n}")
    tol = BCE_TOL[regime]
    for labels in R.BCE_LABELS:
        x, y = R.bce_inputs(n, regime, labels, seed=n + len(labels))
        x_d, y_d = _d(x), _d(y)
        for pw in R.BCE_POS_WEIGHT:
            tag = f"{labels} pw{pw}"
            loss_ref, dx_ref = R.bce_with_logits(x.double(), y.double(), pw)
            loss, dx, ok = _bce(x_d, y_d, pw, n)
            fig.true(f"{tag}: nothing written outside loss / dx", ok)
            fig.close(f"{tag} loss", loss, loss_ref.reshape(1), tol)
            fig.close(f"{tag} n dx", dx * n, dx_ref * n, tol)
            if YARD:
                l32, d32 = R.bce_with_logits(x, y, pw)
                fig.yard(f"{tag} loss", l32.reshape(1), loss_ref.reshape(1))
                fig.yard(f"{tag} n dx", d32 * n, dx_ref * n)
            dxc = dx.cpu()
            fig.true(f"{tag}: loss and dx are finite", bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dxc).all()))
            fig.true(f"{tag}: dx <= 0 where y = 1 and dx >= 0 where y = 0", bool((dxc[y == 1] <= 0).all()) and bool((dxc[y == 0] >= 0).all()))
            loss2, _, ok2 = _bce(x_d, y_d, pw, n, with_dx=False)
            fig.true(f"{tag}: dlogits = NULL gives the same loss bits", ok2 and torch.equal(loss2, loss))
    fig.done()


# ---- 3. SGD and Adam -------------------------------------------------------------------------------------------------------------------

class _Arena:
    """Tensors carved out of one guarded device buffer whose every other float is -0.0 (tests/train_ends_ref.py carve())."""

    def __init__(self, entries, starts, total, values):
        self.entries, self.starts = entries, starts
        self.buf, self.body = _guarded(total, -0.0)
        self.free = torch.ones(total, dtype=torch.bool)
        for (n, *_), s, v in zip(entries, starts, values):
            self.body[s:s + n] = _d(v)
            self.free[s:s + n] = False
        assert ((self.body.data_ptr() & 15) == 0)

    def ptr(self, k):
        return self.body.data_ptr() + 4 * self.starts[k]

    def get(self, k):
        return self.body[self.starts[k]:self.starts[k] + self.entries[k][0]].cpu()

    def all(self):
        return torch.cat([self.get(k) for k in range(len(self.entries))])

    def gaps_intact(self):
        bits, neg0 = _sign_bits(self.body)
        return _bands_intact(self.buf) and bool((bits.cpu()[self.free] == neg0).all())


def _table(entries, *arenas):
    """The device table of an optimizer launch as mintime_amd/optim.py builds it: (pointers..., numel, first block) int64 rows."""
    rows, block = [], 0
    for k, e in enumerate(entries):
        rows.append(tuple(a.ptr(k) for a in arenas) + (e[0], block))
        block += (e[0] + R.OPT_CHUNK - 1) // R.OPT_CHUNK
    return _d(torch.tensor(rows, dtype=torch.int64)), block


def _opt_values(entries, seed, scaled=False):
    g = _gen(seed)
    vals = []
    for n, *_ in entries:
        v = torch.randn(n, generator=g)
        if scaled:        # gradient scales from 1e-12 to 1e6 within one tensor
            v = v * torch.tensor(R.ADAM_GRAD_SCALES)[torch.arange(n) % len(R.ADAM_GRAD_SCALES)]
        vals.append(v)
    return vals


@pytest.mark.parametrize("wd", R.SGD_WD)
@pytest.mark.parametrize("name", list(R.OPT_TABLES))
def test_sgd_multi_vs_fp64(name, wd):
    """mt_sgd_multi on a hand-built table against torch.optim.SGD in fp64: p and g at independent offsets from a 16-byte boundary (the
    float4 path needs both on it), one to three -0.0 floats between neighbours that must keep their bits, the chunk edges
    4095 / 4096 / 4097, zero-length entries first, in the middle and last; lr = 0 leaves the parameters bit-unchanged."""
    entries = R.OPT_TABLES[name]
    ps, gs, ptot, gtot = R.carve(entries)
    p0, g0 = _opt_values(entries, 1), _opt_values(entries, 2)
    lr = 0.1
    fig = _Figures(f"sgd {name} wd{wd}")
    for this_lr in (0.0, lr):
        pa, ga = _Arena(entries, ps, ptot, p0), _Arena(entries, gs, gtot, g0)
        table, blocks = _table(entries, pa, ga)
        L.check(L.get().mt_sgd_multi(table.data_ptr(), len(entries), blocks, this_lr, wd, L.stream_ptr()), "mt_sgd_multi")
        torch.cuda.synchronize()
        fig.true(f"lr {this_lr}: the floats between the tensors keep their bits", pa.gaps_intact() and ga.gaps_intact())
        fig.true(f"lr {this_lr}: the gradients are not written", torch.equal(ga.all(), torch.cat(g0)))
        if this_lr == 0.0:
            fig.true("lr = 0 leaves the parameters bit-unchanged", torch.equal(pa.all(), torch.cat(p0)))
            continue
        for k, (n, po, go) in enumerate(entries):
            if n:
                fig.close(f"p[{k}] n{n} offsets {po},{go}", pa.get(k), R.sgd_step(p0[k].double(), g0[k].double(), lr, wd), SGD_TOL)
        if YARD:
            fig.yard("p", torch.cat([R.sgd_step(p, g, lr, wd) for p, g in zip(p0, g0)]),
                     torch.cat([R.sgd_step(p.double(), g.double(), lr, wd) for p, g in zip(p0, g0)]))
    fig.done()


@pytest.mark.parametrize("t", R.ADAM_STEPS)
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("decoupled", [0, 1])
@pytest.mark.parametrize("name", list(R.OPT_TABLES))
def test_adam_multi_vs_fp64(name, decoupled, wd, t):
    """mt_adam_multi at step t against torch.optim.Adam / AdamW in fp64 (default betas and eps, the bias corrections passed in as
    mintime_amd/optim.py computes them): p per tensor, m and v per gradient scale (1e-12 .. 1e6 within one tensor: the large elements
    must not hide the small ones); the four arenas keep the bits of every float between their tensors."""
    entries = R.OPT_TABLES[name]
    ps, gs, ptot, gtot = R.carve(entries)
    p0, g0 = _opt_values(entries, 3), _opt_values(entries, 4, scaled=True)
    m0 = [v * 0.1 for v in _opt_values(entries, 5)]
    v0 = [v.abs() * 0.01 for v in _opt_values(entries, 6)]
    lr, (b1, b2), eps = 0.05, (0.9, 0.999), 1e-8
    step_size, bc2_sqrt = R.adam_bias_corrections(lr, t)
    pa, ga, ma, va = _Arena(entries, ps, ptot, p0), _Arena(entries, gs, gtot, g0), _Arena(entries, gs, gtot, m0), _Arena(entries, ps, ptot, v0)
    table, blocks = _table(entries, pa, ga, ma, va)
    L.check(L.get().mt_adam_multi(table.data_ptr(), len(entries), blocks, lr, wd, b1, b2, eps, step_size, bc2_sqrt, decoupled, L.stream_ptr()),
            "mt_adam_multi")
    torch.cuda.synchronize()
    fig = _Figures(f"adam {name} decoupled{decoupled} wd{wd} t{t}")
    fig.true("the floats between the tensors keep their bits", all(a.gaps_intact() for a in (pa, ga, ma, va)))
    fig.true("the gradients are not written", torch.equal(ga.all(), torch.cat(g0)))

    def ref_in(dt):
        outs = [R.adam_step(p.to(dt), g.to(dt), m.to(dt), v.to(dt), lr, wd, t, bool(decoupled)) for p, g, m, v in zip(p0, g0, m0, v0)]
        return [[o[i] for o in outs] for i in range(3)]

    rp, rm, rv = ref_in(torch.float64)
    for k, (n, po, go) in enumerate(entries):
        if n:
            fig.close(f"p[{k}] n{n} offsets {po},{go}", pa.get(k), rp[k], ADAM_TOL)
    scale_of = torch.cat([torch.arange(e[0]) % len(R.ADAM_GRAD_SCALES) for e in entries])
    for si, s in enumerate(R.ADAM_GRAD_SCALES):
        sel = scale_of == si
        fig.close(f"m at gradient scale {s:g}", ma.all()[sel], torch.cat(rm)[sel], ADAM_TOL)
        fig.close(f"v at gradient scale {s:g}", va.all()[sel], torch.cat(rv)[sel], ADAM_TOL)
    if YARD:
        yp, ym, yv = ref_in(torch.float32)
        fig.yard("p", torch.cat(yp), torch.cat(rp))
        for si, s in enumerate(R.ADAM_GRAD_SCALES):
            fig.yard(f"m at gradient scale {s:g}", torch.cat(ym)[scale_of == si], torch.cat(rm)[scale_of == si])
            fig.yard(f"v at gradient scale {s:g}", torch.cat(yv)[scale_of == si], torch.cat(rv)[scale_of == si])
    fig.done()


# ---- 4. the dropout passes ---------------------------------------------------------------------------------------------------------------

def _guarded_planes(rows, cols):
    shape = L.planes_shape(rows, cols)
    numel = shape[0] * shape[1] * shape[2] * shape[3] * shape[4]
    buf, body = _guarded(numel, dtype=torch.bfloat16)
    return buf, body.view(shape)


def _keep_multiplier(shape, g):
    return (torch.rand(shape, generator=g) > 0.3).float() / 0.7


@pytest.mark.parametrize("rows,cols", R.MUL_PLANES_CASES)
def test_mul_planes_is_exact(rows, cols):
    """mt_mul_planes: out == x * m to the bit, the planes == split_planes_blk(x * m) to the bit with their zero padding (columns off
    the 8-column lane width and off the 16-column block included); out = NULL gives the same plane bits."""
    g = _gen(rows + cols)
    x, m = torch.randn(rows, cols, generator=g), _keep_multiplier((rows, cols), g)
    x_d, m_d = _d(x), _d(m)
    want = R.mul(x, m)
    want_planes = L.split_planes_blk(_d(want), rows, cols)
    fig = _Figures(f"mul_planes rows{rows} cols{cols}")
    res = []
    for with_out in (True, False):
        pbuf, planes = _guarded_planes(rows, cols)
        obuf, out = _guarded(rows * cols) if with_out else (None, None)
        L.check(L.get().mt_mul_planes(L.ptr(x_d), L.ptr(m_d), L.ptr(planes), L.ptr(out), rows, cols, L.stream_ptr()), "mt_mul_planes")
        torch.cuda.synchronize()
        fig.true(f"out {'given' if with_out else 'NULL'}: nothing written outside planes / out",
                 _bands_intact(pbuf) and (obuf is None or _bands_intact(obuf)))
        fig.true(f"out {'given' if with_out else 'NULL'}: planes == split_planes_blk(x * m), padding included", torch.equal(planes, want_planes))
        res.append(planes)
        if with_out:
            fig.true("out == x * m exactly", torch.equal(out.reshape(rows, cols).cpu(), want))
    fig.true("out = NULL: same plane bits", torch.equal(res[0], res[1]))
    fig.true("x * m splits exactly", torch.equal(L.planes_to_float(res[0], rows, cols).cpu(), want))
    fig.done()


@pytest.mark.parametrize("n", R.MUL_ADD_N)
def test_mul_add_vs_fp64(n):
    """mt_mul_add: out = r + y * m against fp64; the largest n is one float4 past 8192 * 256, so the grid-stride loop runs a second time."""
    g = _gen(n % 1000)
    y, r = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m = _keep_multiplier((n,), g)
    y_d, m_d, r_d = _d(y), _d(m), _d(r)
    buf, out = _guarded(n)
    L.check(L.get().mt_mul_add(L.ptr(y_d), L.ptr(m_d), L.ptr(r_d), L.ptr(out), n, L.stream_ptr()), "mt_mul_add")
    torch.cuda.synchronize()
    fig = _Figures(f"mul_add n{n}")
    ref = R.mul_add(y.double(), m.double(), r.double())
    fig.true("nothing written outside out", _bands_intact(buf))
    fig.close("out", out, ref, MUL_ADD_TOL)
    fig.close("out, the last float4", out[-4:], ref[-4:], MUL_ADD_TOL)
    if YARD:
        fig.yard("out", R.mul_add(y, m, r), ref)
    fig.done()


def test_mul_add_refusals_write_nothing():
    n = 8
    y, m, r = (torch.ones(n + 4, device=dev) for _ in range(3))
    buf, out = _guarded(n + 4, CANARY)
    lib, st = L.get(), L.stream_ptr()
    fig = _Figures("mul_add refusals")
    fig.true("n % 4 != 0", _sync_rc(lib.mt_mul_add(L.ptr(y), L.ptr(m), L.ptr(r), L.ptr(out), 6, st)) == MT_ERR_ARG)
    for k in range(4):
        args = [t[1:] if i == k else t for i, t in enumerate((y, m, r, out))]
        fig.true(f"pointer {k} off a 16-byte boundary", _sync_rc(lib.mt_mul_add(*(L.ptr(a) for a in args), n, st)) == MT_ERR_ARG)
    fig.true("out keeps its canary", bool((out == CANARY).all()) and _bands_intact(buf))
    fig.done()


@pytest.mark.parametrize("regime", R.GEGLU_REGIMES)
@pytest.mark.parametrize("rows", R.GEGLU_ROWS)
@pytest.mark.parametrize("n_half", R.GEGLU_N_HALF)
def test_geglu_backward_pass_vs_fp64(n_half, rows, regime):
    """mt_geglu_bwd: da and dg, each its own section, against autograd of a * gelu(g) (exact erf) in fp64, with the multiplier and with
    m = NULL; the planes are the converter's split of the fp32 du to the bit, padding zeroed; du = NULL gives the same plane bits.
    (The planes are not added back up: dg of `tails` goes down to ~1e-33, where the third bf16 piece of a value falls below bf16's
    normal range -- in the converter as in this kernel.)"""
    dh, m, u = R.geglu_inputs(rows, n_half, regime, seed=rows + n_half)
    dh_d, m_d, u_d = _d(dh), _d(m), _d(u)
    fig = _Figures(f"geglu_bwd {regime} n_half{n_half} rows{rows}")
    tol = GEGLU_TOL[regime]
    for mult, mult_d, tag in ((m, m_d, "m given"), (None, None, "m NULL")):
        ref = R.geglu_bwd(dh.double(), None if mult is None else mult.double(), u.double())
        pbuf, planes = _guarded_planes(rows, 2 * n_half)
        dbuf, du = _guarded(rows * 2 * n_half)
        L.check(L.get().mt_geglu_bwd(L.ptr(dh_d), L.ptr(mult_d), L.ptr(u_d), L.ptr(planes), L.ptr(du), rows, n_half, L.stream_ptr()), "mt_geglu_bwd")
        torch.cuda.synchronize()
        du = du.reshape(rows, 2 * n_half)
        fig.true(f"{tag}: nothing written outside planes / du", _bands_intact(pbuf) and _bands_intact(dbuf))
        fig.close(f"{tag} da", du[:, :n_half], ref[:, :n_half], tol)
        fig.close(f"{tag} dg", du[:, n_half:], ref[:, n_half:], tol)
        if YARD:
            r32 = R.geglu_bwd(dh, mult, u)
            fig.yard(f"{tag} da", r32[:, :n_half], ref[:, :n_half])
            fig.yard(f"{tag} dg", r32[:, n_half:], ref[:, n_half:])
        fig.true(f"{tag}: planes == split_planes_blk(du), padding included", torch.equal(planes, L.split_planes_blk(du, rows, 2 * n_half)))
        pbuf2, planes2 = _guarded_planes(rows, 2 * n_half)
        L.check(L.get().mt_geglu_bwd(L.ptr(dh_d), L.ptr(mult_d), L.ptr(u_d), L.ptr(planes2), None, rows, n_half, L.stream_ptr()), "mt_geglu_bwd")
        torch.cuda.synchronize()
        fig.true(f"{tag}: du = NULL gives the same plane bits", _bands_intact(pbuf2) and torch.equal(planes2, planes))
    fig.done()


def test_geglu_backward_refusal_writes_nothing():
    rows, n_half = 4, 12
    dh, u = torch.ones(rows, n_half, device=dev), torch.ones(rows, 2 * n_half, device=dev)
    pbuf, planes = _guarded_planes(rows, 2 * n_half)
    dbuf, du = _guarded(rows * 2 * n_half, CANARY)
    rc = _sync_rc(L.get().mt_geglu_bwd(L.ptr(dh), None, L.ptr(u), L.ptr(planes), L.ptr(du), rows, n_half, L.stream_ptr()))
    assert rc == MT_ERR_ARG
    assert bool((du == CANARY).all()) and bool(torch.isnan(planes.float()).all()) and _bands_intact(pbuf) and _bands_intact(dbuf)


# ---- 5. BatchNorm sums in fixed order --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime", R.BN_REGIMES)
@pytest.mark.parametrize("rows,C", R.BN_CASES)
def test_det_bn_sums_vs_fp64(rows, C, regime):
    """mt_det_bn_sums, modes 0 and 1, accumulated onto non-zero fp64 stats between guard bands: the three instantiations (16, 32 and 64
    columns per block), one chunk, exactly one chunk (2048 rows) and three; a second launch gives the same bits."""
    x, z, mi, start = R.bn_inputs(rows, C, regime, seed=rows + C)
    x_d, z_d, mi_d = _d(x), _d(z), _d(mi)
    fig = _Figures(f"bn_sums {regime} rows{rows} C{C} W{R.bn_width(C)}")
    for mode in (0, 1):
        ref = R.bn_sums(x.double(), z.double(), mi.double(), mode, exact=True)
        res = []
        for _ in range(2):
            buf, stats = _guarded(2 * C, dtype=torch.float64)
            stats.copy_(_d(start).reshape(-1))
            L.check(L.get().mt_det_bn_sums(L.ptr(x_d), L.ptr(z_d) if mode else None, L.ptr(mi_d) if mode else None, rows, C, mode, L.ptr(stats),
                                           L.stream_ptr()), "mt_det_bn_sums")
            torch.cuda.synchronize()
            fig.true(f"mode {mode}: nothing written outside stats", _bands_intact(buf))
            res.append(stats.reshape(2, C).cpu())
        got = res[0] - start
        fig.close(f"mode {mode} s1", got[0], ref[0], BN_S1_TOL)
        fig.close(f"mode {mode} s2", got[1], ref[1], BN_S2_TOL[mode])
        if YARD:
            r32 = R.bn_sums(x, z, mi, mode)
            fig.yard(f"mode {mode} s1", r32[0], ref[0])
            fig.yard(f"mode {mode} s2", r32[1], ref[1])
        fig.true(f"mode {mode}: second launch bit-identical", torch.equal(res[0], res[1]))
    fig.done()
