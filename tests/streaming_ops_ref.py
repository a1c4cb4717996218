"""fp64 references, launch geometry and case tables of the streaming 1x1 kernels (csrc/skinny_conv.hip, skinny_wgrad.hip,
skinny_bwd.hip, skinny_se.hip, wide_wgrad.hip) for tests/test_gpu_streaming_ops.py.

The reference functions are the formulas of include/mintime_hip.h (mt_conv1x1_rows, mt_conv1x1_wgrad[_wide], mt_conv1x1_bwd_fused,
mt_se_stage_fused) in plain torch, in the dtype of their inputs: fp64 is the reference, the same call in fp32 the yardstick.
tests/test_streaming_ops_ref_host.py ties them to torch autograd of the composed forward, checks the *_supported restatements
against the library, and asserts from the geometry below that every table entry reaches the branch it exists for.

The geometry restates the HOST side of each launcher (chunk height, grid cap, which chunks a block walks); it is what the section
helpers cut the outputs by and what the reach assertions compute with."""
import torch

# ---- references ----------------------------------------------------------------------------------------------------------------------


def swish(u):
    return u * torch.sigmoid(u)


def swish_grad(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def per_row(t, hw, rows):
    """[images, C] -> [rows, C]: row r takes image r // hw."""
    return t.repeat_interleave(hw, 0)[:rows]


def weight_of(wbuf, w_transposed, Cin, Cout):
    """The logical [Cout, Cin] weight inside a pitched buffer: [Cout, ldw] or, transposed, the forward weight [Cin, ldw]."""
    return wbuf[:Cin, :Cout].t() if w_transposed else wbuf[:Cout, :Cin]


def conv1x1_rows(x, wbuf, w_transposed, Cout, amode=0, x2=None, c0=None, c1=None, c2=None, hw=1, res=None):
    """out = a . W^T (+ res) with a = x | swish(c0 x + c1) * c2[row / hw] | c0 x + c1 x2 + c2; returns out, sum out, sum out^2."""
    rows, Cin = x.shape
    a = x
    if amode == 1:
        a = swish(c0 * x + c1) * per_row(c2, hw, rows)
    elif amode == 2:
        a = c0 * x + c1 * x2 + c2
    out = a @ weight_of(wbuf, w_transposed, Cin, Cout).t()
    if res is not None:
        out = out + res
    return out, out.sum(0), (out * out).sum(0)


def conv1x1_wgrad(du, z, kabc, x, sc=None, sh=None, gate=None, hw=1, dw0=0.0):
    """dw0 + (ka du + kb z + kc)^T a with a = x or swish(sc x + sh) * gate[row / hw] (both the accumulator-resident and the wide kernel)."""
    a = x if gate is None else swish(sc * x + sh) * per_row(gate, hw, x.shape[0])
    return (kabc[0] * du + kabc[1] * z + kabc[2]).t() @ a + dw0


def conv1x1_bwd_fused(du, kabc, x, w, res=None, dw0=0.0):
    """dz = ka du + kb (x W^T) + kc; dx = dz W (+ res); dw = dw0 + dz^T x -- z written out, not folded."""
    dz = kabc[0] * du + kabc[1] * (x @ w.t()) + kabc[2]
    dx = dz @ w
    return (dx if res is None else dx + res), dz.t() @ x + dw0


def se_stage(du_p, z_p, kabc, w, zd, scale, shift, mode, hw, gate=None, dpooled=None, mi=None, dgate0=0.0):
    """da = (ka du_p + kb z_p + kc) W;  mode 0: dgate0 + per-image sums of da swish(u);  mode 1: du_d = (da gate + dpooled / hw) swish'(u)
    and its two BatchNorm-backward sums (sum du_d, sum du_d (zd - mean) invstd); u = zd scale + shift."""
    rows, C = zd.shape
    da = (kabc[0] * du_p + kabc[1] * z_p + kabc[2]) @ w
    u = zd * scale + shift
    if mode == 0:
        return ((da * swish(u)).reshape(rows // hw, hw, C).sum(1) + dgate0,)
    dud = (da * per_row(gate, hw, rows) + per_row(dpooled, hw, rows) / hw) * swish_grad(u)
    return dud, dud.sum(0), (dud * (zd - mi[0]) * mi[1]).sum(0)


# ---- the *_supported predicates as the header and the instance lists define them ---------------------------------------------------------

ROWS_INSTANCES = {(1, 1), (1, 3), (1, 5), (3, 1)}                     # (Cin tiles, Cout tiles); all 128-row chunks
# (Cout tiles, Cin tiles) -> (rows per chunk, wave groups along Cout, along Cin, resident blocks per CU, coefficients in registers)
WGRAD_INSTANCES = {(1, 1): (128, 1, 1, 2, 1), (1, 2): (64, 1, 1, 2, 1), (2, 1): (64, 1, 1, 2, 1), (2, 2): (64, 1, 1, 2, 1),
                   (3, 1): (64, 1, 1, 2, 1), (1, 3): (64, 1, 1, 2, 1), (4, 1): (64, 1, 1, 2, 1), (1, 4): (64, 1, 1, 2, 1),
                   (5, 1): (32, 1, 1, 2, 1), (1, 5): (32, 1, 1, 2, 1), (2, 3): (32, 2, 1, 2, 1), (3, 2): (32, 1, 2, 2, 1),
                   (2, 4): (32, 1, 4, 2, 0), (4, 2): (32, 4, 1, 2, 0), (2, 5): (32, 2, 1, 1, 0), (5, 2): (32, 1, 2, 1, 0),
                   (2, 8): (32, 1, 4, 2, 0), (8, 2): (32, 4, 1, 2, 0)}
WIDE_TILES = (3, 4, 6, 10)


def tiles(c):
    return (c + 31) // 32


def rows_built(Cin, Cout):
    return Cin > 0 and Cout > 0 and Cin % 4 == 0 and (tiles(Cin), tiles(Cout)) in ROWS_INSTANCES


def rows_supported(Cin, Cout, amode):
    if not rows_built(Cin, Cout):
        return False
    return amode == 2 or (amode == 0 and (tiles(Cin), tiles(Cout)) == (1, 5))


def wgrad_supported(Cout, Cin):
    return Cout > 0 and Cin > 0 and Cout % 4 == 0 and Cin % 4 == 0 and (tiles(Cout), tiles(Cin)) in WGRAD_INSTANCES


def wide_supported(Cout, Cin):
    return Cout % 4 == 0 and Cin % 4 == 0 and 65 <= Cout <= 320 and 224 <= Cin <= 2048 and tiles(Cout) in WIDE_TILES


def fused_supported(Cout, Cin):
    return Cout in (96, 144) and Cin % 4 == 0 and 0 < Cin <= 32


def fused_instance(Cout, Cin):
    return (3, Cin == 16) if Cout == 96 else (5, False)


def se_supported(Co, C, hw):
    return 0 < Co <= 32 and Co % 4 == 0 and hw > 0 and hw % 64 == 0 and C in (32, 96, 144)


# ---- launch geometry -------------------------------------------------------------------------------------------------------------------


def cdiv(a, b):
    return -(-a // b)


class Walk:
    """Which chunks (of R rows) each block of a launch walks: strided (block b: b, b + grid, ...) or contiguous ranges of `per`."""

    def __init__(self, rows, R, grid, per=None):
        self.rows, self.R, self.grid, self.per = rows, R, grid, per
        self.nchunks = cdiv(rows, R)

    def chunks_of(self, b):
        if self.per is None:
            return list(range(b, self.nchunks, self.grid))
        return list(range(b * self.per, min((b + 1) * self.per, self.nchunks)))

    def counts(self):
        return [len(self.chunks_of(b)) for b in range(self.grid)]

    def later_rows(self):
        """Row mask of every chunk that is not the first one its block walks."""
        m = torch.zeros(self.rows, dtype=torch.bool)
        if self.per is None:
            m[self.grid * self.R:] = True
        else:
            for b in range(self.grid):
                for c in self.chunks_of(b)[1:]:
                    m[c * self.R:(c + 1) * self.R] = True
        return m


def rows_walk(rows):
    return Walk(rows, 128, min(cdiv(rows, 128), 512))


def wgrad_walk(rows, Cout, Cin):
    R, _, _, bpc, _ = WGRAD_INSTANCES[(tiles(Cout), tiles(Cin))]
    return Walk(rows, R, min(cdiv(rows, R), 256 * bpc))


def wgrad_row_groups(Cout, Cin):
    _, wm, wn, _, _ = WGRAD_INSTANCES[(tiles(Cout), tiles(Cin))]
    return 4 // (wm * wn)


def fused_walk(rows, cus):
    return Walk(rows, 64, min(cdiv(rows, 64), cus))


def se_walk(rows):
    n = cdiv(rows, 64)
    grid = min(n, 512)
    return Walk(rows, 64, grid, cdiv(n, grid))


def wide_plan(rows, C, cus):
    """(nslab, nsplit, chunks_per_split, nchunks) of mt_conv1x1_wgrad_wide: 32-row chunks, 128-column slabs, contiguous row ranges."""
    nchunks, nslab = cdiv(rows, 32), cdiv(C, 128)
    nsplit = 8 * max(1, cus // (8 * nslab))
    if nsplit > nchunks:
        nsplit = cdiv(nchunks, 8) * 8
    return nslab, nsplit, cdiv(nchunks, nsplit), nchunks


def wide_walk(rows, C, cus):
    _, nsplit, cps, _ = wide_plan(rows, C, cus)
    return Walk(rows, 32, nsplit, cps)


def wide_rows_for(C, cus, cps):
    """Rows that give `cps` chunks per split at C columns on `cus` CUs, the last range shorter than the others, a ragged last chunk."""
    nsplit = 8 * max(1, cus // (8 * cdiv(C, 128)))
    return (nsplit * (cps - 1) + nsplit // 2 + 1) * 32 - 13


def images_in_chunk(walk, hw, chunk):
    r0 = chunk * walk.R
    r1 = min(r0 + walk.R, walk.rows)
    return (r1 - 1) // hw - r0 // hw + 1


# ---- sections --------------------------------------------------------------------------------------------------------------------------


def row_sections(walk):
    """Named row ranges / masks of a [rows, C] output: first and last 32-row tile of chunk 0, the ragged tail chunk, later chunks."""
    rows, R = walk.rows, walk.R
    s = [("rows: all", slice(0, rows)), ("rows: first tile", slice(0, min(32, rows)))]
    if rows >= R > 32:
        s.append(("rows: last tile of chunk 0", slice(R - 32, R)))
    if rows % R and rows > R:
        s.append(("rows: ragged tail chunk", slice(rows - rows % R, rows)))
    later = walk.later_rows()
    if bool(later.any()):
        s.append(("rows: later chunks of a block", later))
    return s


def col_sections(C, slab=None):
    """The last partial 32-column tile (and, for the wide kernel, the last 128-column slab)."""
    s = []
    if C % 32:
        s.append(("last partial column tile", slice(C - C % 32, C)))
    if slab is not None:
        s.append(("last slab", slice((cdiv(C, slab) - 1) * slab, C)))
    return s


def image_sections(n_img):
    return [(f"image {i}", i) for i in sorted({0, n_img // 2, n_img - 1})]


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
BIG = 10 ** 6        # an hw above every row count of the tables

# mt_conv1x1_rows: (Cin, Cout, amode, rows, hw, ldw - row, w_transposed, residual, stats forms)
ROWS_CASES = [
    (4, 1, 0, 1, 1, 0, 0, False, (0, 1)),
    (16, 16, 0, 31, 1, 4, 0, True, (1, -8)),
    (24, 96, 2, 127, 1, 0, 1, True, (8,)),
    (28, 129, 0, 128, 1, 3, 1, False, (32, -32)),
    (32, 144, 2, 129, 1, 8, 0, True, (-8,)),
    (72, 16, 2, 129, 1, 4, 1, False, (-32,)),
    (96, 1, 0, 127, 1, 0, 0, True, (8,)),
    (96, 16, 0, 31, 1, 5, 0, False, (0,)),
    (16, 96, 1, 257, 1, 0, 0, False, (8,)),              # gate: one image per row
    (24, 144, 1, 300, 7, 4, 0, True, (-8,)),             # 18+ images inside a 128-row chunk
    (32, 16, 1, 300, 49, 0, 1, False, (32,)),            # 3 images inside a chunk
    (96, 16, 1, 385, 128, 0, 0, False, (1,)),            # hw = the chunk height
    (4, 65, 1, 200, BIG, 3, 1, True, (0,)),              # hw > rows: one image
    (28, 65, 2, 1, 1, 0, 1, True, (0,)),
    (16, 96, 2, 512 * 128 + 128 + 77, 1, 0, 1, True, (8, -8)),        # blocks 0 and 1 walk two chunks; slot index wraps
]

_WG_ROWS = lambda R: (1, R - 1, R + 1, 3 * R + 5)
_WG_HW = lambda R: (1, 7, 49, R, BIG)


def _wgrad_small():
    out = []
    for i, ((mt, nt), inst) in enumerate(sorted(WGRAD_INSTANCES.items())):
        R = inst[0]
        gated = i % 2 == 0 or i >= 13                       # 12 gated cases: every hw of _WG_HW at least twice
        out.append((32 * mt - 12, 32 * nt - 20, _WG_ROWS(R)[i % 4], _WG_HW(R)[i % 5] if gated else 0))
    return out


# mt_conv1x1_wgrad: (Cout, Cin, rows, hw or 0 = plain)
WGRAD_CASES = _wgrad_small() + [
    (20, 28, 512 * 128 + 128 + 9, 49),        # R 128, 4 row groups
    (44, 12, 512 * 64 + 64 + 9, 0),           # R 64, 4 row groups
    (148, 12, 512 * 32 + 32 + 9, 32),         # R 32, 4 row groups; hw = the chunk height
    (52, 76, 512 * 32 + 32 + 9, 0),           # R 32, 2 row groups (LDS meeting)
    (40, 144, 256 * 32 + 32 + 9, 7),          # ... one resident block per CU
    (52, 108, 512 * 32 + 32 + 9, 49),         # R 32, 1 row group
]


def wide_cases(cus):
    """mt_conv1x1_wgrad_wide: (Cout, Cin, rows, hw, what the rows are for)."""
    w = lambda C, cps: wide_rows_for(C, cus, cps)
    return [(68, 224, w(224, 1), 32, "cps1"), (80, 240, w(240, 2), 49, "cps2"), (112, 672, w(672, 3), 196, "cps3"),
            (100, 1152, w(1152, 4), 49, "cps4"), (192, 2048, w(2048, 2), 32, "cps2"), (164, 240, w(240, 5), 49, "cps5"),
            (320, 672, w(672, 3), 49, "cps3"), (292, 1152, w(1152, 4), 196, "cps4"), (192, 672, 31, 49, "idle"),
            (320, 2048, w(2048, 1), 32, "cps1")]


def fused_rows(cus, mix, tail):
    """Rows for which the blocks of one launch walk `mix` and `mix + 1` chunks of 64 rows, the last chunk holding `tail` rows."""
    return (mix * cus + cus // 2 - 1) * 64 + tail


def fused_cases(cus):
    """mt_conv1x1_bwd_fused: (Cout, Cin, rows, residual)."""
    f = lambda mix, tail: fused_rows(cus, mix, tail)
    return [(96, 4, 1, False), (96, 16, 64, True), (96, 20, f(1, 1), True), (96, 24, f(1, 63), False), (96, 32, f(4, 1), True),
            (96, 16, f(4, 63), False), (96, 16, f(1, 1), True), (144, 8, f(1, 63), True), (144, 16, f(1, 1), False),
            (144, 24, f(4, 63), True), (144, 32, 1, True)]


# mt_se_stage_fused: (Co, C, hw, images, stats forms of mode 1); every case runs both modes
SE_CASES = [
    (24, 144, 64, 2, (8, -8)),               # the small one
    (4, 96, 128, 5, (1, -8)),
    (16, 32, 64, 1040, (8, -8)),             # 1040 chunks on 512 blocks: ranges of 3 chunks = 3 images, the in-loop flush runs twice
    (32, 96, 192, 200, (32, -32)),           # 600 chunks, ranges of 2 against 3 chunks per image: every second range straddles
    (24, 144, 192, 180, (8, -32)),           # 540 chunks, ranges of 2
    (32, 32, 64, 3, (8,)),
    (4, 144, 64, 3, (-8,)),
    (16, 96, 64, 2, (8,)),
]
