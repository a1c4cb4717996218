"""What tests/test_gpu_gemm_ops.py (GPU) and tests/test_gemm_ref_host.py (CPU) share: the cases, their inputs, the section-wise
comparison and the gates.  No GPU is needed to import or use this module.

A Case names one mt_gemm call.  build(case) draws its operands ON THE CPU as the engines pass them: every matrix is a column slice, at
a non-zero 16-byte aligned offset, of a wider noise-filled tensor (leading dimension = width + 8 floats), every output is such a slice
of a tensor whose other columns hold SLICE_CANARY.  reference(case) evaluates tests/gemm_ref.py on those tensors in fp64, once per
case (cached, never modified).  Cases with a summed output (STATS, the ACT_BWD sums, col_sum, SE_RED) draw operands with a positive
mean, so that no reported sum cancels (test_gemm_ref_host.py asserts |S| >= 0.05 sum|v_i| for every column of every case).

The im2col forms (Case.conv) gather one operand from an image, which has no leading dimension: it is a dense NHWC tensor, fp32 or uint8,
at element IMG_OFF of a longer noise-filled allocation (Built.flat).  The packed weights of the forward cases are ordinary pitched slices
whose columns from k k C on hold the same noise as the rest, so a kernel that multiplies past k k C shows; the weight gradients start
from CANARY and must leave it, exactly, in those columns.  test_gemm_ref_host.py shows that the case list tells six planted mistakes of
a gather from the reference."""
import functools
from dataclasses import dataclass, field, replace

import torch

from . import gemm_ref as R
from .gemm_ref import (OP_NT, OP_NN, OP_TN, PRO_NONE, PRO_BN_SWISH_GATE, PRO_BN_BWD, PRO_IM2COL, BPRO_NONE, BPRO_BN_SWISH_GATE,
                       BPRO_IM2COL, ACT_NONE, ACT_RELU, EPI_STORE, EPI_BIAS_RES, EPI_GEGLU, EPI_STATS, EPI_ATOMIC, EPI_GEGLU_BWD, EPI_ACCUM, EPI_SE_RED, EPI_ACT_BWD)

F64 = torch.float64
CANARY = 7.0            # initial value of accumulated outputs (the reference adds it)
SLICE_CANARY = 5.0      # the columns of an output's wider tensor that the call must not touch
PAD, OFF = 8, 4         # every pitched tensor: leading dimension = width + PAD, slice at column OFF (both multiples of 4 floats)
IMG_OFF = 16            # a gathered image starts at this element of its allocation (16 bytes of uint8, 64 of fp32)
HIGH_BOUND = 3.1 * 2.0 ** -16          # include/mintime_hip.h, MT_PRECISION_HIGH: |error| <= 3.1 * 2^-16 * sum|a||b|

# Gates.  Every figure is max|got - ref| / max|ref| over ONE section (sections()); gate = 2 x the worst case measured on an MI355X over
# every comparison of tests/test_gpu_gemm_ops.py that uses the key, one significant digit up (the factor covers the run-to-run
# variation of atomic summation order and nothing else).  Beside it: the measured worst case (figure, case), and the yardstick -- the
# same reference evaluated in fp32 torch on the CPU against fp64, worst section of that case.
# The "high.*" keys (MT_PRECISION_HIGH on the split-operand loop) are FRACTIONS of the header's bound, evaluated per element from the
# reference operands: max over the section of |got - ref| / (3.1 * 2^-16 * (|a| @ |b|) + TOL[the highest-tier key] * max|ref|).
TOL = {
    "store": 1e-6,          # 4.516e-7 (first row tile, dma3 NT store+bias 64x64x128); yardstick 4.069e-7
    "l2.store": 7e-6,       # 3.030e-6 (interior, l2 NT store 2116x132x4100: 4100 products per element); yardstick 7.956e-7
    # (the im2col forward cases up to K 196 reach 6.268e-7 -- last row tile, cfg3 generic 12x15x4 k7, NT 96x24x196 -- yardstick 5.765e-7:
    #  stored results do not vary from run to run, and the key stays as it is)
    "im2col.store": 3e-6,   # 1.132e-6 (first row tile, cfg3 im2col granule 5x7x64 k3 p2, NT 126x32x576: 576 products per element on the fp32 pipe; the one im2col forward case that does not fit "store"); yardstick 6.588e-7
    "atomic": 1e-6,         # 4.541e-7 (first row tile, bpro b_hw49 split 0, TN 40x72x147); yardstick 4.541e-7
    # (the im2col weight gradients reach 6.931e-7 -- first row tile, one-tile 9x11x8 k5 split 1, TN 32x200x297, a single K range: the
    #  same in every run -- yardstick 6.931e-7: the fp32 rounding of the BN_BWD operand, not of the summation; the key stays as it is.
    #  The split_k 3 and auto cases add their K ranges in the order they finish: over six runs 8 of their 74 sections moved at all, by
    #  1.9e-8 at the most -- one-tile 7x9x32 k3 split 3 -- and none passed 6.931e-7: the margin left under the gate is 16 x that spread)
    "fused": 2e-6,          # 5.372e-7 (worst image, dma_pro3 act_bwd NN 4200x72x96; twice that is 1.07e-6); yardstick 5.372e-7
    "sums": 4e-7,           # 1.620e-7 (sum du xhat, inner columns, act_bwd e_hw1 NN 133x136x36, slots 8); yardstick 1.375e-7
    # (the im2col STATS cases reach 1.886e-7 -- sum of squares, first column tile, cfg0 granule 5x7x64 k3 p2, NT 126x32x576 -- yardstick
    #  1.281e-7: fp64 slots, the same in every run; the key stays as it is)
    "split.store": 2e-6,    # 6.667e-7 (first column tile, S_BIG NN store 1032x264x520); yardstick 7.193e-7
    "split.atomic": 2e-6,   # 5.182e-7 (last row tile, bn_bwd TN atomic 136x248x8200); yardstick 1.633e-7
    "split.fused": 2e-6,    # 5.167e-7 (da last column tile, split NN geglu_bwd 1032x256x520); yardstick 3.333e-7
    "split.sums": 5e-7,     # 2.274e-7 (col_sum dg, inner columns, split NT geglu_bwd 1032x256x520; 2.15e-7 in another run); yardstick 1.886e-7
    "high.store": 0.07,     # 0.03173 of the bound (interior, bn_bwd NN bias_res 1032x264x520); yardstick 0.005059
    "high.atomic": 0.07,    # 0.03231 of the bound (interior, S_BIG NN atomic split 3, 1032x264x520); yardstick 0.004516
    "high.fused": 0.2,      # 0.05929 of the bound (worst image, gate NT store 4116x72x256; twice that is 0.119); yardstick 0.003577
    "high.sums": 0.02,      # 0.009856 of the bound (sum of squares, the one column tile, gate NT stats 4116x72x256); yardstick 0.002612
}
# no gate looser than what tests/test_gpu_gemm.py already accepts for the same kind of quantity: 2e-5 stored results, 5e-5 split-K /
# atomic and fused-epilogue results, 1e-4 column sums; tier high: the whole of the header's bound (plus the highest gate), no more
_CEILING = {"store": 2e-5, "atomic": 5e-5, "fused": 5e-5, "sums": 1e-4}
assert all(v <= (1.0 if k.startswith("high.") else _CEILING[k.split(".")[-1]]) for k, v in TOL.items())


@dataclass(frozen=True)
class Case:
    name: str
    op: int
    M: int
    N: int
    K: int
    pro: int = PRO_NONE
    epi: int = EPI_STORE
    bpro: int = BPRO_NONE
    bias: bool = False
    inplace: bool = False           # BIAS_RES with R == C
    hw: int = 1                     # BN_SWISH_GATE
    b_hw: int = 1                   # BPRO_BN_SWISH_GATE
    e_hw: int = 0                   # SE_RED / ACT_BWD
    n_half: int = 0                 # GEGLU pair
    split_k: int = 1
    slots: int = 8
    a_map: tuple = (0, 0, 0)
    b_map: tuple = (0, 0, 0)
    c_map: tuple = (0, 0, 0)
    tile: tuple = (128, 128)        # (bm, bn) of the kernel variant the case reaches: the sections' tile size
    env: tuple = ()                 # ((name, value), ...) switches the GPU test sets with monkeypatch.setenv
    split: bool = False             # the split-operand pipe is on
    tier: str = "highest"
    long_k: bool = False            # thousands of fp32 products per element on the fp32 pipe: its own gate ("l2.")
    seed: int = 0
    conv: tuple = ()                # im2col forms: (H, W, C, Ho, Wo, k, stride, pad, act) of the gathered operand (A of NT, B of TN)
    src: str = "f32"                # im2col forms: the image's kind, "f32" or "u8"
    affine: bool = False            # im2col forms: the gather carries a per-channel scale / shift

    @property
    def taps(self):                 # k k C: the im2col matrix's columns that hold image data
        return self.conv[5] * self.conv[5] * self.conv[2]

    @property
    def summed(self):
        return self.epi in (EPI_STATS, EPI_GEGLU_BWD, EPI_SE_RED, EPI_ACT_BWD)

    @property
    def c_cols(self):
        return {EPI_GEGLU: self.n_half, EPI_GEGLU_BWD: 2 * self.n_half}.get(self.epi, self.N)

    @property
    def c_rows(self):                # logical rows of C
        return (self.M - 1) // self.e_hw + 1 if self.epi == EPI_SE_RED else self.M

    @property
    def kind(self):
        """TOL key of C."""
        base = ("atomic" if self.epi == EPI_ATOMIC else
                "fused" if self.epi in (EPI_GEGLU, EPI_GEGLU_BWD, EPI_SE_RED, EPI_ACT_BWD) or self.pro == PRO_BN_SWISH_GATE or
                self.bpro not in (BPRO_NONE, BPRO_IM2COL) else "store")
        if self.pro == PRO_IM2COL and self.K >= 512:       # hundreds of fp32 products per element: the im2col forward's own gate
            return "im2col." + base
        return self.prefix + base

    @property
    def prefix(self):
        if self.long_k:
            return "l2."
        return "" if not self.split else ("high." if self.tier == "high" else "split.")


@dataclass
class Built:
    case: Case
    wide: dict = field(default_factory=dict)     # name -> CPU fp32 tensor as allocated (2-D: [rows, width + PAD]; 1-D vectors as they are)
    cols: dict = field(default_factory=dict)     # name -> width of the slice (2-D tensors only)
    outputs: tuple = ()                          # names of the tensors the call writes
    kw: dict = field(default_factory=dict)       # keyword arguments of gemm(); tensors by NAME
    flat: dict = field(default_factory=dict)     # name -> (first element, elements) of a dense operand inside its 1-D allocation (im2col images)

    def views(self, tensors):
        """name -> the operand as the call receives it, from name -> tensor laid out like self.wide (any device / dtype)."""
        def view(k, t):
            if k in self.flat:
                return t[self.flat[k][0]:self.flat[k][0] + self.flat[k][1]]
            return t if k not in self.cols else t[:, OFF:OFF + self.cols[k]]
        return {k: view(k, t) for k, t in tensors.items()}

    def call(self, fn, v, **over):
        """fn(op, A, B, C, M, N, K, lda, ldb, ldc, **kw) with the tensors of `v` (from views()); `over` replaces keyword arguments."""
        c = self.case
        kw = {}
        for k, val in self.kw.items():
            if k == "epi":
                kw[k] = tuple(v.get(x) if isinstance(x, str) else x for x in val)
            else:
                kw[k] = v.get(val) if isinstance(val, str) else val
        kw.update(over)
        # a gathered image has no leading dimension: the engines pass the virtual matrix's width
        ld = lambda n: self.wide[n].shape[1] if n not in self.flat else (c.K if n == "A" else c.N)
        return fn(c.op, v["A"], v["B"], v["C"], c.M, c.N, c.K, ld("A"), ld("B"), ld("C"), **kw)


def _mapped_rows(rmap, rows):
    return int(R.map_rows(rmap, rows).max()) + 1


def build(case):
    c = case
    g = torch.Generator().manual_seed(1234 + c.seed)
    b = Built(c)
    pos = c.summed or c.pro == PRO_IM2COL            # a convolution's forward is drawn once for STORE and STATS

    def image(name, rows):
        """The gathered operand as the engines pass it: a dense NHWC image (fp32 around 1, or uint8 over the whole range) at element
        IMG_OFF of a longer noise-filled 1-D allocation, and the optional per-channel affine (the shift mostly positive, so that
        act(shift) != 0 where a kernel lets the padding through the affine)."""
        H, W, C, Ho, Wo = c.conv[:5]
        assert rows % (Ho * Wo) == 0
        numel = rows // (Ho * Wo) * H * W * C
        if c.src == "u8":
            b.wide[name] = torch.randint(0, 256, (IMG_OFF + numel + 64,), generator=g, dtype=torch.uint8)
        else:
            b.wide[name] = randn(IMG_OFF + numel + 64, mean=1.0, std=0.5)
        b.flat[name] = (IMG_OFF, numel)
        pre = "" if name == "A" else "b_"
        if c.affine:
            b.wide[pre + "scale"], b.wide[pre + "shift"] = rand(C) + 0.5, randn(C, mean=0.5, std=0.5)
            b.kw.update({pre + "scale": pre + "scale", pre + "shift": pre + "shift"})
        b.kw["conv"] = c.conv + (1 if c.src == "u8" else 0,)

    def randn(*shape, mean=0.0, std=1.0):
        return torch.randn(*shape, generator=g) * std + mean

    def rand(*shape):
        return torch.rand(*shape, generator=g)

    def pitched(name, rows, cols, mean=0.0, std=1.0):
        b.wide[name], b.cols[name] = randn(rows, cols + PAD), cols          # unit noise around the slice
        b.wide[name][:, OFF:OFF + cols] = randn(rows, cols, mean=mean, std=std)

    def output(name, rows, cols, fill):
        w = torch.full((rows, cols + PAD), SLICE_CANARY)
        w[:, OFF:OFF + cols] = fill
        b.wide[name], b.cols[name] = w, cols
        b.outputs += (name,)

    M, N, K = c.M, c.N, c.K
    am = 1.0 if pos else 0.0
    wm, ws = (1.0, 0.5) if pos else (0.0, 1.0)
    # ---- A (and A2): NT / NN [M, K], TN [K, M]; rows through a_map
    a_rows, a_cols = (_mapped_rows(c.a_map, K), M) if c.op == OP_TN else (_mapped_rows(c.a_map, M), K)
    if c.pro == PRO_BN_SWISH_GATE:
        pitched("A", a_rows, a_cols)
        b.wide["scale"], b.wide["shift"] = rand(K) + 0.5, rand(K) + 0.5
        b.wide["gate"] = torch.sigmoid(randn((M - 1) // c.hw + 1, K))
        b.kw.update(prologue=c.pro, scale="scale", shift="shift", gate="gate", hw=c.hw)
    elif c.pro == PRO_BN_BWD:
        ch = M if c.op == OP_TN else K
        pitched("A", a_rows, a_cols, mean=am, std=0.5 if pos else 1.0)
        pitched("A2", a_rows, a_cols)
        b.wide["scale"], b.wide["shift"], b.wide["gate"] = rand(ch) + 0.5, randn(ch, std=0.1), rand(ch) * 0.5 + 0.25
        b.kw.update(prologue=c.pro, scale="scale", shift="shift", gate="gate", A2="A2")
    elif c.pro == PRO_IM2COL:
        image("A", M)
        b.kw.update(prologue=c.pro)
    else:
        pitched("A", a_rows, a_cols, mean=am, std=0.5 if pos else 1.0)
    # ---- B: NT [N, K], NN / TN [K, N] (rows through b_map)
    inv = K ** -0.5
    if c.op == OP_NT:
        pitched("B", N, K, mean=wm * inv, std=ws * inv)
    elif c.bpro == BPRO_BN_SWISH_GATE:
        pitched("B", _mapped_rows(c.b_map, K), N)
        b.wide["b_scale"], b.wide["b_shift"] = rand(N) + 0.5, rand(N) + 0.5
        b.wide["b_gate"] = torch.sigmoid(randn((K - 1) // c.b_hw + 1, N))
        b.kw.update(b_prologue=c.bpro, b_scale="b_scale", b_shift="b_shift", b_gate="b_gate", b_hw=c.b_hw)
    elif c.bpro == BPRO_IM2COL:
        image("B", K)
        b.kw.update(b_prologue=c.bpro)
    else:
        pitched("B", _mapped_rows(c.b_map, K), N, mean=wm * inv, std=ws * inv)
    # ---- C and the epilogue's extras
    c_rows_mem = _mapped_rows(c.c_map, c.c_rows) + (2 if c.epi == EPI_SE_RED else 0)      # SE_RED: two rows past the last image, not to be touched
    if c.epi in (EPI_ATOMIC, EPI_ACCUM):
        fill = CANARY
    elif c.epi == EPI_SE_RED:
        fill = 0.0
    elif c.inplace:
        fill = randn(c_rows_mem, c.c_cols)
    else:
        fill = float("nan")
    output("C", c_rows_mem, c.c_cols, fill)
    b.kw.update(epilogue=c.epi, split_k=c.split_k, a_map=c.a_map, b_map=c.b_map, c_map=c.c_map)
    if c.bias:
        b.wide["bias"] = randn(N)
        b.kw["bias"] = "bias"
    if c.epi == EPI_BIAS_RES:
        if c.inplace:
            b.kw.update(R="C", ldr=c.c_cols + PAD)
        else:
            pitched("R", c_rows_mem, N)
            b.kw.update(R="R", ldr=N + PAD)
    if c.epi in (EPI_STATS, EPI_ACT_BWD):
        b.kw.update(stats="stats", stats_slots=c.slots)
        b.outputs += ("stats",)
    if c.epi == EPI_GEGLU:
        output("C2", M, 2 * c.n_half, float("nan"))
        b.kw.update(C2="C2", ldc2=2 * c.n_half + PAD, n_half=c.n_half)
    if c.epi == EPI_GEGLU_BWD:
        pitched("C2", M, 2 * c.n_half, mean=1.0)
        b.wide["col_sum"] = torch.full((2 * c.n_half,), CANARY)
        b.outputs += ("col_sum",)
        b.kw.update(C2="C2", ldc2=2 * c.n_half + PAD, n_half=c.n_half, col_sum="col_sum")
    if c.epi in (EPI_SE_RED, EPI_ACT_BWD):
        n_img = (M - 1) // c.e_hw + 1
        pitched("C2", M, N)
        # u = z e_scale + e_shift around 2 +- 0.7: swish(u) and swish'(u) keep their sign, so that not even a 5-row image's sum cancels
        b.wide["e_scale"], b.wide["e_shift"] = rand(N) * 0.4 + 0.3, rand(N) + 1.5
        b.wide["e_gate"] = torch.sigmoid(randn(n_img, N))
        b.wide["e_dpool"] = randn(n_img, N, mean=1.0, std=0.3) * c.e_hw
        b.wide["e_mi"] = torch.cat((randn(N, mean=-1.0, std=0.1), rand(N) + 0.5))
        act = c.epi == EPI_ACT_BWD
        b.kw.update(C2="C2", ldc2=N + PAD,
                    epi=("e_scale", "e_shift", "e_gate" if act else None, "e_dpool" if act else None, "e_mi" if act else None, c.e_hw))
    return b


@functools.lru_cache(maxsize=None)
def built(case):
    """build() once per case (the tier, the pipe and the environment switches do not change the inputs)."""
    return build(case)


def _input_key(case):
    return replace(case, name="", env=(), split=False, tier="highest", tile=(0, 0), slots=8, long_k=False)


@functools.lru_cache(maxsize=None)
def _reference(key, dtype):
    b = built(key)
    v = b.views({k: t.to(dtype) for k, t in b.wide.items()})
    v["stats"] = None
    out = b.call(R.gemm, v)
    return out


@functools.lru_cache(maxsize=None)
def _bound(key):
    b = built(key)
    v = b.views({k: t.double() for k, t in b.wide.items()})
    a, bb = b.call(lambda *p, **kw: R.operands(*p[:3], *p[4:9], **kw), v)
    return HIGH_BOUND * (a.abs() @ bb.abs())


def inputs(case):
    return built(_input_key(case))


def reference(case, dtype=F64):
    """{name: tensor} of tests/gemm_ref.py for the case, in `dtype` arithmetic.  Shared by every test that runs the same inputs: do
    not modify."""
    return _reference(_input_key(case), dtype)


def high_bound(case):
    """The header's per-element bound of tier high on the case's product: HIGH_BOUND * (|a| @ |b|), [M, N] fp64, from the reference
    operands after their prologues."""
    return _bound(_input_key(case))


# ---- section-wise comparison -------------------------------------------------------------------------------------------------------

def _ranges(n, tile):
    """[(name, slice)] of the first tile, the last tile (when there are two) and what lies between (when there are three)."""
    tiles = (n + tile - 1) // tile
    out = [("first", slice(0, min(tile, n)))]
    if tiles > 1:
        out.append(("last", slice((tiles - 1) * tile, n)))
    if tiles > 2:
        out.append(("inner", slice(tile, (tiles - 1) * tile)))
    return out


def _figure(d, r, floor=None, tol0=0.0):
    den = max(float(r.abs().max()), 1e-30)
    if floor is None:
        return float(d.max()) / den
    return float((d / (floor + tol0 * den)).max())


def sections(got, ref, bm, bn, hw=0, floor=None, tol0=0.0):
    """[(section, figure)] of a [rows, cols] result against its reference: first / last row tile (all columns), first / last column
    tile (all rows), the interior (neither), and with hw > 0 the worst single image of hw rows.  figure = max|got - ref| / max|ref|
    over the section; with `floor` (a per-element error bound) max of |got - ref| / (floor + tol0 max|ref|)."""
    g, r = got.detach().cpu().double(), ref.double()
    assert g.shape == r.shape, (g.shape, r.shape)
    d = (g - r).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    rows, cols = r.shape
    rr, cr = dict(_ranges(rows, bm)), dict(_ranges(cols, bn))
    fl = (lambda rs, cs: None) if floor is None else (lambda rs, cs: floor[rs, cs])
    out = []
    al = slice(None)
    for k in ("first", "last"):
        if k in rr:
            out.append((f"{k} row tile", _figure(d[rr[k]], r[rr[k]], fl(rr[k], al), tol0)))
    for k in ("first", "last"):
        if k in cr:
            out.append((f"{k} column tile", _figure(d[:, cr[k]], r[:, cr[k]], fl(al, cr[k]), tol0)))
    if "inner" in rr and "inner" in cr:
        out.append(("interior", _figure(d[rr["inner"], cr["inner"]], r[rr["inner"], cr["inner"]], fl(rr["inner"], cr["inner"]), tol0)))
    if hw > 0:
        worst = max(_figure(d[i:i + hw], r[i:i + hw], fl(slice(i, i + hw), al), tol0) for i in range(0, rows, hw))
        out.append(("worst image", worst))
    return out


def sum_sections(got, ref, bn, floor=None, tol0=0.0):
    """[(section, figure)] of a vector of column sums [cols]: first / last column tile and the columns between."""
    g, r = got.detach().cpu().double().reshape(1, -1), ref.double().reshape(1, -1)
    d = (g - r).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    names = {"first": "first column tile", "last": "last column tile", "inner": "inner columns"}
    return [(names[k], _figure(d[:, s], r[:, s], None if floor is None else floor.reshape(1, -1)[:, s], tol0))
            for k, s in _ranges(r.shape[1], bn)]


def condition(out):
    """{name: min over the columns of |S| / sum|v_i|} for every summed output of a reference (gemm_ref's `*_abs` entries); col_sum
    without the canary it started from."""
    res = {}
    for k, sabs in out.items():
        if k.endswith("_abs"):
            s = out[k[:-4]]
            if k == "col_sum_abs":
                s = s - CANARY
            res[k[:-4]] = float((s.abs() / sabs.clamp_min(1e-300)).min())
    return res


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

CFG_TILES = [(128, 128), (128, 64), (256, 32), (64, 64)]                      # csrc/gemm.hip kCfg, MT_FORCE_CFG 0..3
DMA_VARS = [(128, 128, 32, 2), (128, 128, 16, 3), (128, 64, 16, 3), (64, 64, 32, 3), (64, 64, 16, 3)]    # csrc/gemm_dma.hip kVar


def cfg_cases(cfg):
    """(a) the four register-staged tiles: three row tiles (the last of 4 rows) by two column tiles (the last of 4 columns) at K 36,
    one exact tile, and 4 x 4 x 4."""
    bm, bn = CFG_TILES[cfg]
    kw = dict(tile=(bm, bn), env=(("MT_FORCE_CFG", str(cfg)),))
    M, N, K = 2 * bm + 4, bn + 4, 36
    t = f"cfg{cfg}"
    cs = [Case(f"{t} NT store+bias", OP_NT, M, N, K, bias=True, seed=1, **kw),
          Case(f"{t} NT bias_res in place", OP_NT, M, N, K, epi=EPI_BIAS_RES, bias=True, inplace=True, seed=2, **kw),
          Case(f"{t} NT stats", OP_NT, M, N, K, epi=EPI_STATS, seed=3, **kw),
          Case(f"{t} NN store", OP_NN, M, N, K, seed=4, **kw),
          Case(f"{t} NN accum", OP_NN, M, N, K, epi=EPI_ACCUM, seed=5, **kw),
          Case(f"{t} TN atomic split 1", OP_TN, M, N, K, epi=EPI_ATOMIC, split_k=1, seed=6, **kw),
          Case(f"{t} TN atomic split 3", OP_TN, M, N, K, epi=EPI_ATOMIC, split_k=3, seed=6, **kw)]
    for (m, n, k) in ((bm, bn, 36), (4, 4, 4)):
        cs += [Case(f"{t} NT store+bias {m}x{n}x{k}", OP_NT, m, n, k, bias=True, seed=7, **kw),
               Case(f"{t} NN store {m}x{n}x{k}", OP_NN, m, n, k, seed=8, **kw),
               Case(f"{t} TN atomic split 1 {m}x{n}x{k}", OP_TN, m, n, k, epi=EPI_ATOMIC, seed=9, **kw)]
    if cfg == 3:      # a row-mapped atomic output (one K range: deterministic mode refuses split-K into mapped rows, csrc/det.hip)
        cs.append(Case(f"{t} TN atomic c_map", OP_TN, M, N, K, epi=EPI_ATOMIC, c_map=(20, 21, 1), seed=10, **kw))
    return cs


def l2_cases():
    """(a) L2-blocked tile order on the 64 x 64 tile: 34 row tiles (XCD bands of 5 and 4 rows: padding blocks), 3 column tiles.
    K 4092: tile_grid gives group_n = 2 (2 MB / (64 * 4092 * 4 B) = 2.002), the last group one tile wide; K 4100: group_n = 1."""
    kw = dict(tile=(64, 64), env=(("MT_FORCE_CFG", "3"),), long_k=True)
    return [Case(f"l2 NT store K{k}", OP_NT, 33 * 64 + 4, 132, k, seed=11, **kw) for k in (4092, 4100)]


def gate_pro_cases(hw):
    """(a) NT BN_SWISH_GATE below M 4096 (register-staged; N 72 -> the 128 x 128 tile): image boundaries inside a tile."""
    M = {1: 133, 9: 15 * 9, 49: 3 * 49}[hw]
    return [Case(f"gate hw{hw} NT {'stats' if e == EPI_STATS else 'store'}", OP_NT, M, 72, 36, pro=PRO_BN_SWISH_GATE, epi=e, hw=hw,
                 seed=12) for e in (EPI_STORE, EPI_STATS)]


def bn_bwd_cases(K):
    """(a) BN_BWD prologue, register-staged, K % 16 in {4, 8, 12}: kc != 0 must not reach the zero-filled k-tail.  N 68 pads to
    128 columns with either tile width: pick_cfg takes the 128 x 128 tile."""
    return [Case(f"bn_bwd K{K} NN store", OP_NN, 133, 68, K, pro=PRO_BN_BWD, seed=13),
            Case(f"bn_bwd K{K} NN bias_res", OP_NN, 133, 68, K, pro=PRO_BN_BWD, epi=EPI_BIAS_RES, seed=14),
            Case(f"bn_bwd K{K} TN atomic", OP_TN, 132, 68, K, pro=PRO_BN_BWD, epi=EPI_ATOMIC, split_k=2, seed=15)]


def bpro_cases(b_hw):
    """(a) TN BN_BWD + BPRO_BN_SWISH_GATE (the project conv's weight gradient): K = n_img * b_hw rows, M 40 x N 72 -> 128 x 128."""
    K = {1: 37, 9: 15 * 9, 49: 3 * 49}[b_hw]
    return [Case(f"bpro b_hw{b_hw} split {s}", OP_TN, 40, 72, K, pro=PRO_BN_BWD, bpro=BPRO_BN_SWISH_GATE, epi=EPI_ATOMIC, b_hw=b_hw,
                 split_k=s, seed=16) for s in (0, 3)]


def se_cases(e_hw):
    """(a) SE_RED / ACT_BWD on the register-staged kernels (M < 4096; N 40 and 136 both take the 128 x 64 tile)."""
    M = {1: 133, 5: 53 * 5, 49: 7 * 49, 200: 2 * 200}[e_hw]
    cs = []
    for N in (40, 136):
        for K in (16, 36):
            kw = dict(pro=PRO_BN_BWD, e_hw=e_hw, tile=(128, 64), seed=17)
            cs.append(Case(f"se_red e_hw{e_hw} N{N} K{K}", OP_NN, M, N, K, epi=EPI_SE_RED, **kw))
            cs += [Case(f"act_bwd e_hw{e_hw} N{N} K{K} slots {s}", OP_NN, M, N, K, epi=EPI_ACT_BWD, slots=s, **kw) for s in (8, -8)]
    return cs


def geglu_bwd_cases(n_half):
    """(a) GEGLU_BWD, NT over W2^T and NN over W2, register-staged (K 36), 64 x 64 tile (pick_cfg: CFG_SMALL)."""
    kw = dict(epi=EPI_GEGLU_BWD, n_half=n_half, tile=(64, 64))
    return [Case(f"geglu_bwd NT n_half{n_half}", OP_NT, 133, n_half, 36, seed=18, **kw),
            Case(f"geglu_bwd NN n_half{n_half}", OP_NN, 133, n_half, 36, seed=19, **kw)]


def dma_cases(v):
    """(b) the five LDS-DMA variants: ring prologue deeper than, equal to and shallower than the K loop."""
    bm, bn, bk, st = DMA_VARS[v]
    cs = []
    for K in (bk, 2 * bk, (st + 1) * bk):
        for (M, N) in ((bm + 4, bn + 4), (64, 64)):
            kw = dict(tile=(bm, bn), env=(("MT_DMA_VARIANT", str(v)),))
            t = f"dma{v} {M}x{N}x{K}"
            cs += [Case(f"{t} NT store+bias", OP_NT, M, N, K, bias=True, seed=20, **kw),
                   Case(f"{t} NN store", OP_NN, M, N, K, seed=21, **kw),
                   Case(f"{t} TN atomic split 2", OP_TN, M, N, K, epi=EPI_ATOMIC, split_k=2, seed=22, **kw)]
    return cs


def dma_pro_cases(v):
    """(b) SE_RED / ACT_BWD on the LDS-DMA prologue kernels (M >= 4096, K % 16 == 0); 65 / 66 row tiles: the L2-blocked order.
    Variants 2 and 4 (bk 16) at K 16 and 48.  Variant 3 is the bk 32, two-stage kernel, which try_launch_dma keeps only for
    K % 32 == 0 (any other K is rewritten to variant 4): K 32 and 96, the ring equal to and shallower than the K loop."""
    bm, bn = DMA_VARS[v][:2]
    cs = []
    for (M, e_hw) in ((84 * 49, 49), (21 * 200, 200)):
        for K in ((32, 96) if DMA_VARS[v][2] == 32 else (16, 48)):
            kw = dict(pro=PRO_BN_BWD, e_hw=e_hw, tile=(bm, bn), env=(("MT_DMA_PRO_VARIANT", str(v)),), seed=23)
            cs += [Case(f"dma_pro{v} se_red M{M} K{K}", OP_NN, M, 72, K, epi=EPI_SE_RED, **kw),
                   Case(f"dma_pro{v} act_bwd M{M} K{K}", OP_NN, M, 72, K, epi=EPI_ACT_BWD, **kw)]
    return cs


def split_cases(tier):
    """(c) the split-operand loop at the smallest eligible shapes (csrc/gemm_split_dispatch.hpp)."""
    big, mid, wg = (1032, 264, 520), (3656, 72, 512), (136, 248, 8200)
    kb = dict(tile=(128, 128), split=True, tier=tier)
    km = dict(tile=(128, 64), split=True, tier=tier)
    return [Case("S_BIG NT store+bias", OP_NT, *big, bias=True, seed=30, **kb),
            Case("S_BIG NT bias_res in place", OP_NT, *big, epi=EPI_BIAS_RES, bias=True, inplace=True, seed=31, **kb),
            Case("S_BIG NN store", OP_NN, *big, seed=32, **kb),
            Case("S_BIG NN accum", OP_NN, *big, epi=EPI_ACCUM, seed=33, **kb),
            Case("S_BIG NN atomic split 3", OP_NN, *big, epi=EPI_ATOMIC, split_k=3, seed=34, **kb),
            Case("S_MID NT store", OP_NT, *mid, seed=35, **km),
            Case("S_MID NN store", OP_NN, *mid, seed=36, **km),
            Case("TN xcd-k split 0", OP_TN, *wg, epi=EPI_ATOMIC, split_k=0, seed=37, **kb),
            Case("TN plain split 4", OP_TN, *wg, epi=EPI_ATOMIC, split_k=4, seed=37, **kb),
            Case("TN a_map split 0", OP_TN, *wg, epi=EPI_ATOMIC, split_k=0, a_map=(40, 41, 1), seed=38, **kb),
            Case("bn_bwd NN store", OP_NN, *big, pro=PRO_BN_BWD, seed=39, **kb),
            Case("bn_bwd NN bias_res", OP_NN, *big, pro=PRO_BN_BWD, epi=EPI_BIAS_RES, seed=40, **kb),
            Case("bn_bwd TN atomic", OP_TN, *wg, pro=PRO_BN_BWD, epi=EPI_ATOMIC, split_k=0, seed=41, **kb),
            # gate prologue: 128 x 64 only where 64-wide tiles pad fewer columns (N 72 pads to 128 either way -> 128 x 128; N 192 -> 128 x 64)
            Case("gate NT stats", OP_NT, 4116, 72, 256, pro=PRO_BN_SWISH_GATE, epi=EPI_STATS, hw=49, seed=42, **kb),
            Case("gate NT store", OP_NT, 4116, 72, 256, pro=PRO_BN_SWISH_GATE, epi=EPI_STORE, hw=49, seed=42, **kb),
            Case("gate NT stats N192", OP_NT, 4116, 192, 256, pro=PRO_BN_SWISH_GATE, epi=EPI_STATS, hw=49, seed=43, **km),
            Case("gate NT store N192", OP_NT, 4116, 192, 256, pro=PRO_BN_SWISH_GATE, epi=EPI_STORE, hw=49, seed=43, **km)]


def extra_cases():
    """Forms the dispatchers can launch that the lists above do not reach, at small shapes: the split-K atomic NT / NN and GEGLU on
    the register-staged kernels (K 36); the LDS-DMA kernels' other epilogues at the variant pick_variant gives them (pipe off,
    132 x 132 x 64: NT / STATS 64 x 64, NT atomic and GEGLU_BWD 128 x 64, NN atomic and GEGLU 128 x 128); the split-operand loop's
    NT atomic, STATS (from M 4096), GEGLU and GEGLU_BWD at tier highest."""
    d, s = dict(seed=50), dict(split=True, seed=51)
    return [Case("reg NT atomic+bias split 3", OP_NT, 133, 68, 36, epi=EPI_ATOMIC, bias=True, split_k=3, **d),
            Case("reg NN atomic split 2", OP_NN, 133, 68, 36, epi=EPI_ATOMIC, split_k=2, **d),
            Case("reg NT geglu", OP_NT, 133, 128, 36, epi=EPI_GEGLU, bias=True, n_half=64, **d),
            Case("dma NT bias_res", OP_NT, 132, 132, 64, epi=EPI_BIAS_RES, bias=True, tile=(64, 64), **d),
            Case("dma NT stats", OP_NT, 132, 132, 64, epi=EPI_STATS, tile=(64, 64), **d),
            Case("dma NT atomic+bias split 2", OP_NT, 132, 132, 64, epi=EPI_ATOMIC, bias=True, split_k=2, tile=(128, 64), **d),
            Case("dma NN accum", OP_NN, 132, 132, 64, epi=EPI_ACCUM, tile=(64, 64), **d),
            Case("dma NN atomic split 2", OP_NN, 132, 132, 64, epi=EPI_ATOMIC, split_k=2, **d),
            Case("dma NT geglu", OP_NT, 132, 128, 64, epi=EPI_GEGLU, bias=True, n_half=64, **d),
            Case("dma NT geglu_bwd", OP_NT, 132, 64, 64, epi=EPI_GEGLU_BWD, n_half=64, tile=(128, 64), **d),
            Case("dma NN geglu_bwd", OP_NN, 132, 64, 64, epi=EPI_GEGLU_BWD, n_half=64, tile=(128, 64), **d),
            Case("split NT atomic+bias split 2", OP_NT, 1032, 264, 520, epi=EPI_ATOMIC, bias=True, split_k=2, **s),
            Case("split NT stats", OP_NT, 4104, 72, 512, epi=EPI_STATS, tile=(128, 64), **s),
            Case("split NT geglu", OP_NT, 1032, 512, 520, epi=EPI_GEGLU, bias=True, n_half=256, **s),
            Case("split NT geglu_bwd", OP_NT, 1032, 256, 520, epi=EPI_GEGLU_BWD, n_half=256, tile=(128, 64), **s),
            Case("split NN geglu_bwd", OP_NN, 1032, 256, 520, epi=EPI_GEGLU_BWD, n_half=256, tile=(128, 64), **s)]


# ---- the im2col forms ---------------------------------------------------------------------------------------------------------------

def _pad4(n):
    return (n + 3) // 4 * 4


# A side (NT): (kind, n, H, W, C, k, s, p, Ho, Wo, Cout, affine, act, sources).  The smallest shapes that reach each edge:
IM2COL_A = [
    # M 627: ragged last row tile at 64, 128 and 256; 72 columns: ragged at 32, 64 and 128; act(shift) != 0 at the padding
    ("granule", 3, 11, 19, 8, 3, 1, 1, 11, 19, 72, True, ACT_RELU, ("f32",)),
    ("granule", 2, 13, 18, 4, 5, 2, 2, 7, 9, 40, True, ACT_NONE, ("f32",)),          # 25-bit tap mask, stride 2 on an odd H
    ("granule", 2, 5, 7, 64, 3, 1, 2, 7, 9, 32, False, ACT_NONE, ("f32",)),          # K 576: the "full" correlation of a data gradient
    ("granule", 2, 4, 6, 4, 3, 1, 3, 8, 10, 16, True, ACT_RELU, ("f32",)),           # padding >= k: whole windows outside the image
    ("granule", 3, 9, 12, 64, 1, 2, 0, 5, 6, 136, True, ACT_RELU, ("f32",)),         # strided 1 x 1 skip convolution
    ("generic", 2, 10, 14, 3, 3, 2, 0, 5, 7, 32, False, ACT_NONE, ("f32", "u8")),    # Ho = ceil(H / 2) at pad 0: the SAME overhang; K 28
    ("generic", 2, 9, 13, 3, 3, 2, 1, 5, 7, 32, False, ACT_NONE, ("f32", "u8")),     # odd sizes, leading pad 1
    ("generic", 2, 9, 13, 3, 3, 2, 0, 4, 6, 32, False, ACT_NONE, ("f32", "u8")),     # valid padding
    ("generic", 2, 12, 15, 4, 7, 2, 3, 6, 8, 24, True, ACT_RELU, ("f32",)),          # k k = 49 > 32 leaves the granule form; K 196
]


def _geo(H, W, C, k, s, p, Ho, Wo):
    return f"{H}x{W}x{C} k{k} s{s} p{p} -> {Ho}x{Wo}"


def im2col_a_cases(cfg):
    """MT_PRO_IM2COL (NT) with EPI_STORE and EPI_STATS on the tile MT_FORCE_CFG = cfg forces; granule form (fp32, C % 4 == 0,
    k k <= 32) and generic form (3 channels, uint8, k k > 32)."""
    bm, bn = CFG_TILES[cfg]
    cs = []
    for i, (kind, n, H, W, C, k, s, p, Ho, Wo, Cout, aff, act, srcs) in enumerate(IM2COL_A):
        for src in srcs:
            for e in (EPI_STORE, EPI_STATS):
                cs.append(Case(f"cfg{cfg} im2col {kind} {src} {_geo(H, W, C, k, s, p, Ho, Wo)} {'stats' if e == EPI_STATS else 'store'}",
                               OP_NT, n * Ho * Wo, Cout, _pad4(k * k * C), pro=PRO_IM2COL, epi=e, conv=(H, W, C, Ho, Wo, k, s, p, act),
                               src=src, affine=aff, tile=(bm, bn), env=(("MT_FORCE_CFG", str(cfg)),), seed=60 + i))
    return cs


# B side (TN, BN_BWD + ATOMIC onto CANARY): (group, H, W, C, k, s, p, Ho, Wo, Cout, affine, act, sources, tile); Ho and Wo are given, as
# on the A side (10 x 14 at pad 0 -> 5 x 7 is the SAME overhang).  Three images each; Ho Wo is odd wherever the geometry leaves the
# choice (3 x 16 and the valid stem geometry are 48 and 24 pixels), so that an image boundary falls inside a 16-pixel k-step.  The tile
# is the one gemm.hip picks: 128 x 128 for 72 columns, 256 x 32 for 28, the one-tile 64 x 288 for Cout <= 64 and 192 < columns <= 288,
# 128 x 64 for 288 columns at Cout 68 and for 192 columns (test_gemm_ref_host.py asks the library).
IM2COL_B = [
    ("granule", 5, 7, 8, 3, 1, 1, 5, 7, 72, True, ACT_RELU, ("f32",), (128, 128)),          # Wo 7: below the k-step
    ("granule", 3, 16, 8, 3, 1, 1, 3, 16, 72, True, ACT_RELU, ("f32",), (128, 128)),        # Wo 16: the k-step
    ("granule", 3, 17, 8, 3, 1, 1, 3, 17, 72, True, ACT_RELU, ("f32",), (128, 128)),        # Wo 17: just above it
    ("granule", 3, 37, 8, 3, 1, 1, 3, 37, 72, True, ACT_RELU, ("f32",), (128, 128)),        # Wo 37: more than twice it
    ("granule", 9, 13, 8, 3, 2, 1, 5, 7, 72, True, ACT_RELU, ("f32",), (128, 128)),         # stride 2, Wo 7
    ("one-tile", 7, 9, 32, 3, 1, 0, 5, 7, 64, True, ACT_RELU, ("f32",), (64, 288)),         # 288 columns, Cout 64
    ("one-tile", 9, 11, 8, 5, 1, 2, 9, 11, 32, True, ACT_NONE, ("f32",), (64, 288)),        # 200 columns, Cout 32
    ("ordinary", 7, 9, 32, 3, 1, 0, 5, 7, 68, True, ACT_RELU, ("f32",), (128, 64)),         # Cout 68: just outside the one-tile configuration
    ("ordinary", 9, 13, 192, 1, 2, 0, 5, 7, 64, True, ACT_RELU, ("f32",), (128, 64)),       # 192 columns: just outside it (strided 1 x 1)
    ("generic", 10, 14, 3, 3, 2, 0, 5, 7, 32, False, ACT_NONE, ("f32", "u8"), (256, 32)),
    ("generic", 9, 13, 3, 3, 2, 1, 5, 7, 32, False, ACT_NONE, ("f32", "u8"), (256, 32)),
    ("generic", 9, 13, 3, 3, 2, 0, 4, 6, 32, False, ACT_NONE, ("f32", "u8"), (256, 32)),
    ("generic", 13, 17, 4, 7, 2, 3, 7, 9, 24, True, ACT_RELU, ("f32",), (64, 288)),         # k k = 49: the per-element gather on the one tile
    ("generic", 13, 17, 4, 7, 2, 3, 7, 9, 72, True, ACT_RELU, ("f32",), (128, 128)),        # ... and on the ordinary path
]
IM2COL_B_IMAGES = 3


def im2col_b_cases():
    """MT_BPRO_IM2COL (TN, BN_BWD prologue on A, ATOMIC): the weight gradients, each at split_k 1, 3 and 0 (auto)."""
    cs = []
    for i, (group, H, W, C, k, s, p, Ho, Wo, Cout, aff, act, srcs, tile) in enumerate(IM2COL_B):
        for src in srcs:
            for sk in (1, 3, 0):
                cs.append(Case(f"im2col wgrad {group} {src} {_geo(H, W, C, k, s, p, Ho, Wo)} Cout {Cout} split {sk}", OP_TN, Cout,
                               _pad4(k * k * C), IM2COL_B_IMAGES * Ho * Wo, pro=PRO_BN_BWD, bpro=BPRO_IM2COL, epi=EPI_ATOMIC, split_k=sk,
                               conv=(H, W, C, Ho, Wo, k, s, p, act), src=src, affine=aff, tile=tile, seed=80 + i))
    return cs


def all_gpu_cases():
    cs = []
    for cfg in range(4):
        cs += cfg_cases(cfg) + im2col_a_cases(cfg)
    cs += im2col_b_cases()
    cs += l2_cases()
    for hw in (1, 9, 49):
        cs += gate_pro_cases(hw) + bpro_cases(hw)
    for K in (36, 40, 44):
        cs += bn_bwd_cases(K)
    for e_hw in (1, 5, 49, 200):
        cs += se_cases(e_hw)
    for nh in (64, 192):
        cs += geglu_bwd_cases(nh)
    for v in range(5):
        cs += dma_cases(v)
    for v in (2, 3, 4):
        cs += dma_pro_cases(v)
    for tier in ("highest", "high"):
        cs += split_cases(tier)
    return cs + extra_cases()
