"""The 3-D convolution of csrc/conv3d.hip as include/mintime_hip.h defines it, in plain torch on the CPU: the reference side of
tests/test_gpu_conv3d_ops.py, and the tables of its cases.  Every function computes in the dtype of its operands: float64 is the
reference, float32 the yardstick.  Written from the header's three formulas

    fwd:   y[m][co]        = sum over taps, ci of  pro(x)[in(m, tap)][ci] * w[co][tap][ci]
    dgrad: dx[r][ci]       = sum over taps, co of  dy[out(r, tap)][co] * wt[tap][co][ci]
    wgrad: dw[co][tap][ci] = sum over m of         dy[m][co] * pro(x)[in(m, tap)][ci]

with in(m, tap) the input row that tap (a, b, c) of output position (n, to, ho, wo) reads, (n, to st - pt + a, ho sh - ph + b,
wo sw - pw + c), nothing outside the volume; out(r, tap) the output row that read input position (n, t, h, w) through that tap,
((t + pt - a) / st, ...) where the stride divides and the quotient is on the output grid, else nothing; and
pro(v) = relu(v scale + shift), applied to the input's values only -- the padding stays zero.  The loops run over the taps, one
index vector per tap: slow, and meant for the sizes of the tables below.  tests/test_conv3d_ref_host.py ties the three to
torch.nn.functional.conv3d and its autograd, and proves that every table entry reaches the branch it was chosen for."""
from collections import namedtuple

import torch


class Geo(namedtuple("Geo", "N T H W C K k s p")):
    """One convolution: input grid and channels, output channels, (kt, kh, kw), stride and padding per axis."""
    __slots__ = ()

    @property
    def out(self):
        return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((self.T, self.H, self.W), self.k, self.s, self.p))

    @property
    def taps(self):
        return self.k[0] * self.k[1] * self.k[2]

    @property
    def rows_in(self):
        return self.N * self.T * self.H * self.W

    @property
    def rows_out(self):
        To, Ho, Wo = self.out
        return self.N * To * Ho * Wo

    def tap(self, i):
        """tap index -> (a, b, c), c fastest: the order of the packed weights."""
        kt, kh, kw = self.k
        return i // (kh * kw), (i // kw) % kh, i % kw


def geo(case):
    """A table entry (name, C, K, k, s, p, (N, T, H, W)) as a Geo."""
    _, C, K, k, s, p, (N, T, H, W) = case
    return Geo(N, T, H, W, C, K, tuple(k), tuple(s), tuple(p))


# ---- layouts ----------------------------------------------------------------------------------------------------------------------

def pack_w(w, cin):
    """torch weight [K, C, kt, kh, kw] -> [K][kt][kh][kw][cin] as [K, taps * cin]; cin >= C appends zero input channels."""
    K, C = w.shape[:2]
    out = torch.zeros(K, w.shape[2], w.shape[3], w.shape[4], cin, dtype=w.dtype)
    out[..., :C] = w.permute(0, 2, 3, 4, 1)
    return out.reshape(K, -1)


def unpack_w(wp, K, C, k):
    """[K, taps * C] -> torch layout [K, C, kt, kh, kw]."""
    return wp.reshape(K, *k, C).permute(0, 4, 1, 2, 3)


def pack_wt(w):
    """torch weight [K, C, kt, kh, kw] -> [kt][kh][kw][K][C] as [taps * K, C]."""
    return w.permute(2, 3, 4, 0, 1).reshape(-1, w.shape[1]).clone()


def rows(t, ld=None, fill=float("nan")):
    """[N, C, T, H, W] -> the channels-last rows [N*T*H*W, ld]: columns [0, C) hold the data, the gap [C, ld) holds `fill`."""
    C = t.shape[1]
    r = t.permute(0, 2, 3, 4, 1).reshape(-1, C)
    if ld is None or ld == C:
        return r.clone()
    out = torch.full((r.shape[0], ld), fill, dtype=t.dtype)
    out[:, :C] = r
    return out


def unrows(r, N, T, H, W, C):
    """rows [N*T*H*W, ld >= C] -> [N, C, T, H, W]."""
    return r[:, :C].reshape(N, T, H, W, C).permute(0, 4, 1, 2, 3)


# ---- the index form -----------------------------------------------------------------------------------------------------------------

def _grid(N, T, H, W):
    m = torch.arange(N * T * H * W)
    return m // (T * H * W), (m // (H * W)) % T, (m // W) % H, m % W


def in_index(g, tap):
    """in(m, tap) for every output row m: the input row, or -1 outside the volume."""
    To, Ho, Wo = g.out
    a, b, c = g.tap(tap)
    n, to, ho, wo = _grid(g.N, To, Ho, Wo)
    ti, hi, wi = to * g.s[0] - g.p[0] + a, ho * g.s[1] - g.p[1] + b, wo * g.s[2] - g.p[2] + c
    inside = (ti >= 0) & (ti < g.T) & (hi >= 0) & (hi < g.H) & (wi >= 0) & (wi < g.W)
    row = ((n * g.T + ti) * g.H + hi) * g.W + wi
    return torch.where(inside, row, torch.full_like(row, -1))


def out_index(g, tap):
    """out(r, tap) for every input row r: the output row that read r through this tap, or -1 (the stride does not divide, or the
    quotient is off the output grid)."""
    To, Ho, Wo = g.out
    a, b, c = g.tap(tap)
    n, t, h, w = _grid(g.N, g.T, g.H, g.W)
    tt, hh, ww = t + g.p[0] - a, h + g.p[1] - b, w + g.p[2] - c
    ok = (tt >= 0) & (hh >= 0) & (ww >= 0) & (tt % g.s[0] == 0) & (hh % g.s[1] == 0) & (ww % g.s[2] == 0)
    to, ho, wo = tt // g.s[0], hh // g.s[1], ww // g.s[2]
    ok = ok & (to < To) & (ho < Ho) & (wo < Wo)
    row = ((n * To + to) * Ho + ho) * Wo + wo
    return torch.where(ok, row, torch.full_like(row, -1))


def pro(x, scale, shift):
    """BatchNorm + ReLU of the producer, folded: relu(x scale + shift) per channel; scale None = identity."""
    return x if scale is None else torch.clamp_min(x * scale + shift, 0)


def _take(src, idx):
    """src[idx] with zero rows where idx is -1."""
    got = src[idx.clamp_min(0)]
    return got * (idx >= 0).to(src.dtype)[:, None]


def fwd_ref(g, x, wp, scale=None, shift=None):
    """y [rows_out, K] from x [rows_in, C] and wp = pack_w(w, C)."""
    a = pro(x, scale, shift)
    w3 = wp.reshape(g.K, g.taps, g.C)
    y = torch.zeros(g.rows_out, g.K, dtype=x.dtype)
    for tap in range(g.taps):
        y += _take(a, in_index(g, tap)) @ w3[:, tap, :].t()
    return y


def dgrad_ref(g, dy, wt):
    """dx [rows_in, C] (the gradient of pro(x)) from dy [rows_out, K] and wt = pack_wt(w)."""
    w3 = wt.reshape(g.taps, g.K, g.C)
    dx = torch.zeros(g.rows_in, g.C, dtype=dy.dtype)
    for tap in range(g.taps):
        dx += _take(dy, out_index(g, tap)) @ w3[tap]
    return dx


def wgrad_ref(g, x, dy, scale=None, shift=None):
    """dw [K, taps * C] (pack_w's layout) from x [rows_in, C] and dy [rows_out, K]."""
    a = pro(x, scale, shift)
    dw = torch.zeros(g.K, g.taps, g.C, dtype=x.dtype)
    for tap in range(g.taps):
        dw[:, tap, :] = dy.t() @ _take(a, in_index(g, tap))
    return dw.reshape(g.K, -1)


def stats_ref(y):
    """BatchNorm sums of y: [2, K] (sum, sum of squares)."""
    return torch.stack([y.sum(0), (y * y).sum(0)])


# ---- sections -----------------------------------------------------------------------------------------------------------------------

def y_sections(g):
    """Output rows by what their taps see: `border` (at least one tap outside the volume, at least one inside), `interior` (every tap
    inside) and `padding` (no tap inside: the row is exactly zero).  Boolean masks over the output rows."""
    inside = torch.stack([in_index(g, t) >= 0 for t in range(g.taps)])
    return {"interior": inside.all(0), "border": inside.any(0) & ~inside.all(0), "padding": ~inside.any(0)}


def dx_sections(g):
    """Input rows likewise: `unread` (no tap of any output position reads the row: its gradient is exactly zero), `border` (read, but
    some tap would need an output position beyond an edge of the output grid) and `interior`."""
    To, Ho, Wo = g.out
    n, t, h, w = _grid(g.N, g.T, g.H, g.W)
    read = torch.stack([out_index(g, tap) >= 0 for tap in range(g.taps)]).any(0)
    edge = torch.zeros(g.rows_in, dtype=torch.bool)
    for tap in range(g.taps):
        a, b, c = g.tap(tap)
        for v, pp, off, ss, no in ((t, g.p[0], a, g.s[0], To), (h, g.p[1], b, g.s[1], Ho), (w, g.p[2], c, g.s[2], Wo)):
            q = v + pp - off
            edge |= (q < 0) | (q > (no - 1) * ss)
    return {"interior": read & ~edge, "border": read & edge, "unread": ~read}


def zero_taps(g):
    """The taps that lie outside the volume for every output position: their weight gradient is exactly zero."""
    return [t for t in range(g.taps) if not bool((in_index(g, t) >= 0).any())]


# ---- the launcher's split arithmetic -------------------------------------------------------------------------------------------------

BM, BN, BK = 64, 64, 16          # csrc/conv3d.hip: block tile and reduction step


def split_rows(R, splits):
    """(rows per split, splits that get rows) of a weight gradient over R output rows asked to run in `splits` parts: the rows are
    dealt in equal parts rounded up to whole reduction steps of 16, and the parts past the last row do not run."""
    share = (R + splits - 1) // splits
    per = (share + BK - 1) // BK * BK
    return per, (R + per - 1) // per


# ---- case tables: (name, C, K, kernel, stride, padding, (N, T, H, W)) ----------------------------------------------------------------

_ONE, _NOPAD = (1, 1, 1), (0, 0, 0)
# 1x1x1, stride 1: the row counts around the 64-row tile, the channel counts around the 64-column tile and the 16-deep reduction step
TILE_CASES = [
    ("r1_c4_k4", 4, 4, _ONE, _ONE, _NOPAD, (1, 1, 1, 1)),
    ("r63_c20_k36", 20, 36, _ONE, _ONE, _NOPAD, (1, 1, 7, 9)),
    ("r64_c64_k64", 64, 64, _ONE, _ONE, _NOPAD, (1, 1, 8, 8)),
    ("r65_c68_k68", 68, 68, _ONE, _ONE, _NOPAD, (1, 1, 5, 13)),
    ("r129_c132_k132", 132, 132, _ONE, _ONE, _NOPAD, (1, 3, 43, 1)),
    ("r65_c132_k4", 132, 4, _ONE, _ONE, _NOPAD, (1, 1, 5, 13)),
    ("r63_c4_k132", 4, 132, _ONE, _ONE, _NOPAD, (1, 1, 7, 9)),
]
# kh != kw, sh != sw, ph != pw: no two axes can be exchanged unnoticed
ASYM_CASES = [
    ("asym", 8, 12, (3, 2, 5), (2, 1, 3), (1, 0, 2), (2, 5, 6, 11)),
    ("asym2", 4, 8, (2, 3, 1), (1, 2, 2), (1, 1, 0), (2, 3, 7, 6)),
]
PAD_CASES = [
    ("padonly", 8, 8, _ONE, _ONE, (0, 1, 1), (1, 2, 3, 4)),
]
# the network's forms at their temporal and spatial edges
NET_CASES = [
    ("fusion_t9", 8, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0), (2, 9, 3, 3)),
    ("fusion_t1", 8, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0), (2, 1, 3, 3)),
    ("fast_stem", 4, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3), (2, 2, 5, 6)),
    ("conv_a_3", 32, 16, (3, 1, 1), _ONE, (1, 0, 0), (3, 1, 4, 5)),
    ("branch1_s2", 32, 64, _ONE, (1, 2, 2), _NOPAD, (2, 2, 6, 8)),
    ("conv_b_s2", 16, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 6, 8)),
]
CASES = TILE_CASES + ASYM_CASES + PAD_CASES + NET_CASES
# 32769 output rows: 513 blocks of 64, so the statistics take the two-level reduction (chunks of 512 partial rows) with one row in
# the last chunk.  Forward only.
BIG_CASE = ("r32769_c4_k4", 4, 4, _ONE, _ONE, _NOPAD, (1, 1, 1, 32769))

# the weight gradient's splits: output grids (N, To, Ho, Wo) of R rows, each asked for in every count of SPLIT_COUNTS(R)
SPLIT_GRIDS = {1: (1, 1, 1, 1), 16: (2, 2, 2, 2), 17: (1, 1, 1, 17), 33: (1, 1, 3, 11), 100: (2, 2, 5, 5), 504: (2, 3, 7, 12)}
SPLIT_KERNELS = {"1x1x1": (_ONE, _ONE, _NOPAD), "asym": ASYM_CASES[0][3:6]}
SPLIT_C, SPLIT_K = 8, 12


def split_counts(R):
    return [1, 2, 3, 7, 64, R + 5]


def split_case(R, kernel):
    """The table entry whose output grid is SPLIT_GRIDS[R] under SPLIT_KERNELS[kernel]: the smallest input grid that gives it."""
    k, s, p = SPLIT_KERNELS[kernel]
    N, *o = SPLIT_GRIDS[R]
    size = tuple((n - 1) * ss + kk - 2 * pp for n, kk, ss, pp in zip(o, k, s, p))
    return (f"split_r{R}_{kernel}", SPLIT_C, SPLIT_K, k, s, p, (N,) + size)


def inputs(case, seed=0):
    """fp32 operands of a case in torch layout: x [N, C, T, H, W], w [K, C, kt, kh, kw], dy [N, K, To, Ho, Wo], scale and shift [C].
    The shift is strictly positive, so a prologue applied to the padding would turn it into something other than zero."""
    g = geo(case)
    gen = torch.Generator().manual_seed(seed + sum(ord(ch) for ch in case[0]))
    x = torch.randn(g.N, g.C, g.T, g.H, g.W, generator=gen)
    w = torch.randn(g.K, g.C, *g.k, generator=gen) / (g.C * g.taps) ** 0.5
    dy = torch.randn(g.N, g.K, *g.out, generator=gen)
    scale = torch.rand(g.C, generator=gen) + 0.5
    shift = torch.rand(g.C, generator=gen) * 0.5 + 0.25
    return x, w, dy, scale, shift
