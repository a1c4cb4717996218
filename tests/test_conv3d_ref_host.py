"""tests/conv3d_ref.py on the CPU: its three index-form definitions against torch.nn.functional.conv3d and autograd of it in fp64 for
every table entry, the property each table entry was chosen for (so that a later edit of a table cannot drop a branch of
csrc/conv3d.hip silently), the engine's two weight packings against the reference's, and mt_conv3d_wgrad_splits -- a host function of
the library that launches nothing and loads without a device -- by its documented properties."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mintime_amd import lib as L, slowfast_engine as E

from . import conv3d_ref as R
from .test_gpu_slowfast import CONVS
from .util import rel_err

TOL = 1e-12      # fp64: sums of at most ~3e4 O(1) products in two different orders differ by ~1e-14 relative

SPLIT_CASES = [R.split_case(r, kern) for kern in R.SPLIT_KERNELS for r in R.SPLIT_GRIDS]
ALL = R.CASES + SPLIT_CASES
_IDS = [c[0] for c in ALL]
_BY_NAME = {c[0]: c for c in ALL}


def _operands(case):
    g = R.geo(case)
    x, w, dy, scale, shift = (t.double() for t in R.inputs(case))
    return g, x, w, dy, scale, shift


def _bc(v):
    return v[None, :, None, None, None]


@pytest.mark.parametrize("with_pro", [False, True], ids=["plain", "pro"])
@pytest.mark.parametrize("case", ALL, ids=_IDS)
def test_index_forms_are_conv3d_and_its_adjoints(case, with_pro):
    """fwd_ref, dgrad_ref and wgrad_ref from the reference's own packings against F.conv3d of relu(x scale + shift) (the padding
    added by conv3d, so after the activation) and autograd of it, with respect to the activated input and the weight."""
    g, x, w, dy, scale, shift = _operands(case)
    sc, sh = (scale, shift) if with_pro else (None, None)
    a = (F.relu(x * _bc(scale) + _bc(shift)) if with_pro else x).clone().requires_grad_(True)
    wv = w.clone().requires_grad_(True)
    y = F.conv3d(a, wv, stride=g.s, padding=g.p)
    assert tuple(y.shape[2:]) == g.out and y.numel() == g.rows_out * g.K
    y.backward(dy)
    xr, dyr = R.rows(x), R.rows(dy)
    got_y = R.fwd_ref(g, xr, R.pack_w(w, g.C), sc, sh)
    assert rel_err(got_y, R.rows(y.detach())) <= TOL
    assert rel_err(R.unrows(got_y, g.N, *g.out, g.K), y.detach()) <= TOL
    assert rel_err(R.dgrad_ref(g, dyr, R.pack_wt(w)), R.rows(a.grad)) <= TOL
    got_dw = R.wgrad_ref(g, xr, dyr, sc, sh)
    assert rel_err(R.unpack_w(got_dw, g.K, g.C, g.k), wv.grad) <= TOL
    assert rel_err(got_dw, R.pack_w(wv.grad, g.C)) <= TOL
    st = R.stats_ref(got_y)
    assert rel_err(st[0], y.detach().sum((0, 2, 3, 4))) <= TOL and rel_err(st[1], (y.detach() ** 2).sum((0, 2, 3, 4))) <= TOL


def test_big_case_forward_is_conv3d():
    g, x, w, _, scale, shift = _operands(R.BIG_CASE)
    y = F.conv3d(F.relu(x * _bc(scale) + _bc(shift)), w)
    assert g.rows_out == 32769 and rel_err(R.fwd_ref(g, R.rows(x), R.pack_w(w, g.C), scale, shift), R.rows(y)) <= TOL


def test_padding_stays_zero_under_the_prologue():
    """pro(0) = relu(shift) > 0 for every channel of the tables' inputs, so a prologue applied to the padding would show: the rows
    that read nothing but padding are exactly zero, with the prologue and without, and activating the padded tensor instead
    (the wrong order) gives something else."""
    case = _BY_NAME["padonly"]
    g, x, w, _, scale, shift = _operands(case)
    assert bool((shift > 0).all()) and all(bool((R.inputs(c)[4] > 0).all()) for c in ALL)
    pad = R.y_sections(g)["padding"]
    assert int(pad.sum()) == 36 and g.rows_out == 60
    for sc, sh in ((None, None), (scale, shift)):
        y = R.fwd_ref(g, R.rows(x), R.pack_w(w, g.C), sc, sh)
        assert bool((y[pad] == 0).all()) and bool((y[~pad] != 0).all())
    xp = F.pad(x, (g.p[2],) * 2 + (g.p[1],) * 2 + (g.p[0],) * 2)
    wrong = R.rows(F.conv3d(F.relu(xp * _bc(scale) + _bc(shift)), w))
    assert bool((wrong[pad] != 0).any())


def test_layout_helpers():
    t = torch.arange(2 * 3 * 2 * 2 * 5, dtype=torch.float64).reshape(2, 3, 2, 2, 5)
    r = R.rows(t, 8)
    assert r.shape == (40, 8) and bool(torch.isnan(r[:, 3:]).all())
    assert r[(1 * 2 + 1) * 2 * 5 + 1 * 5 + 4, 2] == t[1, 2, 1, 1, 4]              # row ((n T + t) H + h) W + w, column c
    assert torch.equal(R.unrows(r, 2, 2, 2, 5, 3), t) and torch.equal(R.rows(t), r[:, :3])
    assert bool((R.rows(t, 8, fill=7.0)[:, 3:] == 7.0).all())
    w = torch.randn(6, 3, 2, 3, 4, dtype=torch.float64)
    wp = R.pack_w(w, 4).reshape(6, 2, 3, 4, 4)
    assert wp[5, 1, 2, 3, 1] == w[5, 1, 1, 2, 3] and bool((wp[..., 3] == 0).all())
    assert torch.equal(R.unpack_w(R.pack_w(w, 3), 6, 3, (2, 3, 4)), w)
    assert R.pack_wt(w).reshape(2, 3, 4, 6, 3)[1, 0, 3, 4, 2] == w[4, 2, 1, 0, 3]
    g = R.geo(_BY_NAME["asym"])
    assert [g.tap(i) for i in (0, 1, 5, 10, 29)] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (2, 1, 4)]


@pytest.mark.parametrize("K,C,k", [(8, 3, (5, 7, 7)), (12, 8, (3, 2, 5)), (16, 32, (3, 1, 1))])
def test_engine_packings_are_the_headers(K, C, k):
    """slowfast_engine._pack_w / _pack_wt (what the network hands the kernels) and the reference's packings (written from the header)
    describe one layout, the stems' zero fourth channel included."""
    w = torch.randn(K, C, *k)
    cin = (C + 3) // 4 * 4
    assert torch.equal(E._pack_w(w, cin), R.pack_w(w, cin))
    assert torch.equal(E._pack_wt(w), R.pack_wt(w))


# ---- the tables reach what they were chosen for ------------------------------------------------------------------------------------

def test_tile_table_edges():
    gs = [R.geo(c) for c in R.TILE_CASES]
    assert all(g.k == (1, 1, 1) and g.s == (1, 1, 1) and g.p == (0, 0, 0) and g.rows_in == g.rows_out for g in gs)
    assert {g.rows_out for g in gs} == {1, 63, 64, 65, 129}
    assert {g.rows_out: (g.N, g.T, g.H, g.W) for g in gs} == {1: (1, 1, 1, 1), 63: (1, 1, 7, 9), 64: (1, 1, 8, 8), 65: (1, 1, 5, 13),
                                                              129: (1, 3, 43, 1)}
    assert {g.K for g in gs} == {4, 36, 64, 68, 132} and {g.C for g in gs} == {4, 20, 64, 68, 132}
    # forward statistics and weight gradient: a second and a third tile of output channels, each with a partial last row tile
    for K, tiles in ((68, 2), (132, 3)):
        assert any(g.K == K and -(-g.K // R.BN) == tiles and g.rows_out > R.BM and g.rows_out % R.BM for g in gs)
    # weight gradient: a second tile of the taps x C axis
    assert any(g.taps * g.C > R.BN for g in gs)
    # data gradient: a second tile of input channels, and a reduction of taps x K that ends inside a step of 16
    assert any(g.C == 68 and -(-g.C // R.BN) == 2 for g in gs)
    assert {4, 36, 68} <= {g.K for g in gs if (g.taps * g.K) % R.BK}
    # forward: a reduction of taps x C that ends inside a step, and one of several whole steps
    assert any((g.taps * g.C) % R.BK for g in gs) and any((g.taps * g.C) % R.BK == 0 and g.taps * g.C > R.BK for g in gs)


def test_asymmetric_table_edges():
    a, b = (R.geo(c) for c in R.ASYM_CASES)
    # no two axes of asym's kernel, stride or padding are exchangeable; asym2 tells h from w by kernel and padding, t from h by all
    assert all(len(set(v)) == 3 for v in (a.k, a.s, a.p, (a.T, a.H, a.W)))
    assert b.k[1] != b.k[2] and b.p[1] != b.p[2] and b.k[0] != b.k[1] and b.s[0] != b.s[1] and b.H != b.W
    assert a.out == (3, 5, 4) and a.rows_out == 120 and b.out == (4, 4, 3)
    sec = R.dx_sections(b)
    assert b.rows_in == 252 and int(sec["unread"].sum()) == 126
    for g in (a, b):          # every kind of row exists
        ys, xs = R.y_sections(g), R.dx_sections(g)
        assert bool(ys["border"].any()) and bool(ys["interior"].any()) and bool(xs["border"].any()) and bool(xs["interior"].any())
    assert (a.taps * a.K) % R.BK and (a.taps * a.C) % R.BK == 0 and a.taps * a.C > R.BN


def test_network_table_edges():
    g = {c[0]: R.geo(c) for c in R.NET_CASES}
    assert g["fusion_t9"].out == (3, 3, 3) and g["fusion_t1"].out == (1, 3, 3)
    assert len(R.zero_taps(g["fusion_t1"])) == 6 and R.zero_taps(g["fusion_t9"]) == []
    assert len(R.zero_taps(g["fast_stem"])) == 98 and g["fast_stem"].taps == 245
    s = R.dx_sections(g["branch1_s2"])
    assert g["branch1_s2"].rows_in == 192 and int(s["unread"].sum()) == 144
    # the temporal stride of 4 at T = 9: input frames 0..8, of which the stride test alone decides which output frame reads which
    f9 = g["fusion_t9"]
    reads = torch.stack([R.out_index(f9, t) >= 0 for t in range(f9.taps)]).sum(0)
    assert sorted(set(reads.tolist())) == [1, 2]
    # wherever a temporal tap could cross into the neighbouring clip there is a neighbouring clip
    assert all(v.N >= 2 for v in g.values() if v.k[0] > 1)
    assert bool(R.y_sections(g["conv_b_s2"])["border"].any()) and bool(R.dx_sections(g["conv_b_s2"])["border"].any())
    assert g["conv_a_3"].T == 1 and len(R.zero_taps(g["conv_a_3"])) == 2


def test_exact_zero_sections_are_zero_in_the_reference():
    """What the GPU test asserts to be exactly 0.0 is exactly 0.0 in the fp64 reference, and nothing else of the section kinds is."""
    for case in R.CASES:
        g, x, w, dy, scale, shift = _operands(case)
        xr, dyr = R.rows(x), R.rows(dy)
        y = R.fwd_ref(g, xr, R.pack_w(w, g.C), scale, shift)
        assert bool((y[R.y_sections(g)["padding"]] == 0).all())
        dx = R.dgrad_ref(g, dyr, R.pack_wt(w))
        unread = R.dx_sections(g)["unread"]
        assert bool((dx[unread] == 0).all()) and bool((dx[~unread] != 0).any(1).all())
        dw = R.wgrad_ref(g, xr, dyr, scale, shift).reshape(g.K, g.taps, g.C)
        zt = R.zero_taps(g)
        assert all(bool((dw[:, t] == 0).all()) == (t in zt) for t in range(g.taps))


def test_split_table_edges():
    assert R.split_rows(16, 1) == (16, 1) and all(R.split_rows(16, s) == (16, 1) for s in R.split_counts(16))      # dw written directly
    assert R.split_rows(17, 7) == (16, 2)                                                                          # nsplit < splits
    assert R.split_rows(100, 3) == (48, 3) and 100 - 2 * 48 == 4                                                   # a short last split
    assert R.split_rows(504, 3) == (176, 3) and 504 - 2 * 176 == 152 and 152 % R.BK == 8                           # ... ending in a partial step
    assert R.split_rows(1, 6) == (16, 1) and R.split_rows(504, 509) == (16, 32) and R.split_rows(33, 64) == (16, 3)
    for r, grid in R.SPLIT_GRIDS.items():
        assert set(R.split_counts(r)) == {1, 2, 3, 7, 64, r + 5}
        for kern in R.SPLIT_KERNELS:
            g = R.geo(R.split_case(r, kern))
            assert (g.N,) + g.out == grid and g.rows_out == r and (g.C, g.K) == (8, 12)
            assert g.K <= R.BM and (g.taps * g.C <= R.BN or kern == "asym")
        for s in R.split_counts(r):
            per, n = R.split_rows(r, s)
            assert per % R.BK == 0 and 1 <= n <= s and (n - 1) * per < r <= n * per
    assert set(R.SPLIT_GRIDS) == {1, 16, 17, 33, 100, 504}


# ---- mt_conv3d_wgrad_splits ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def handle():
    import os
    if not os.path.exists(L.LIB_PATH):
        L.build()
    h = ctypes.CDLL(L.LIB_PATH)
    h.mt_conv3d_wgrad_splits.argtypes = [ctypes.c_void_p]
    h.mt_conv3d_wgrad_splits.restype = ctypes.c_int
    return h


def _desc(g):
    To, Ho, Wo = g.out
    return L.Conv3dDesc(N=g.N, T=g.T, H=g.H, W=g.W, C=g.C, To=To, Ho=Ho, Wo=Wo, K=g.K, kt=g.k[0], kh=g.k[1], kw=g.k[2], st=g.s[0], sh=g.s[1],
                        sw=g.s[2], pt=g.p[0], ph=g.p[1], pw=g.p[2], ldx=g.C, ldy=g.K)


def _network_geos():
    """Every distinct convolution of the network at full size: 8 clips, 8 (slow) and 32 (fast) frames, 56 x 56 down to 7 x 7, at the
    test table's widths and at 4 and 32 times them (res5's conv_b is 512 -> 512 channels, its conv_c 512 -> 2048)."""
    out = []
    for _, cin, cout, k, s, p in CONVS:
        for mult in (1, 4, 32):
            if cin == 3 and mult > 1:
                continue
            C, K = (4, cout) if cin == 3 else (cin * mult, cout * mult)
            out += [R.Geo(8, T, hw, hw, C, K, k, s, p) for T in (8, 32) for hw in (56, 28, 14, 7)]
    return out


def test_wgrad_splits_properties(handle):
    assert handle.mt_conv3d_wgrad_splits(None) == 1
    geos = [R.geo(c) for c in ALL + [R.BIG_CASE]] + _network_geos()
    seen = set()
    for g in geos:
        d = _desc(g)
        s = handle.mt_conv3d_wgrad_splits(ctypes.byref(d))
        seen.add(s)
        assert 1 <= s <= 4096, (g, s)
        assert s <= -(-g.rows_out // 128), (g, s)                       # at least 8 reduction steps of 16 rows per split
        if s > 1:
            assert s * g.K * g.taps * g.C * 4 <= 256 << 20, (g, s)      # the workspace the caller allocates
    assert 1 in seen and max(seen) > 64                                 # both ends of the range occur
