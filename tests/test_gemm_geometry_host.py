"""CPU-only: the launch geometry of the four GEMM dispatchers (csrc/gemm_geometry.hpp) -- the L2-blocked tile grid and the split-K
ranges -- through the two debug exports beside mt_debug_gemm_trace (not in the header, not in lib.PROTOTYPES; they launch nothing).

Every expected value is a fixed number worked out by hand from the arithmetic the dispatchers carried before they shared one
planner; none is computed by the code under test."""
import ctypes
import os

import pytest

from mintime_amd import lib

PLAIN, XCD, XCD_CAPPED = 0, 1, 2      # gemm_geometry.hpp KForm


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    h = ctypes.CDLL(lib.LIB_PATH)
    out = ctypes.POINTER(ctypes.c_int)
    h.mt_debug_tile_grid.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong, out]
    h.mt_debug_tile_grid.restype = None
    h.mt_debug_split_k.argtypes = [ctypes.c_int] * 6 + [out]
    h.mt_debug_split_k.restype = None
    return h


# (M, N, bm, bn, panel bytes) -> (m_tiles, n_tiles, grid_x, group_n)
TILE_GRID = [
    ((12576, 1536, 128, 128, 128 * 512 * 2 * 3), (99, 12, 1248, 5)),      # plane loop, tier highest: the ragged last group
    ((12576, 1536, 128, 128, 128 * 512 * 2 * 2), (99, 12, 1248, 8)),      # ... tier high: two planes per operand
    ((12576, 4096, 128, 128, 128 * 512 * 2 * 3), (99, 32, 3328, 5)),
    ((12576, 512, 128, 128, 128 * 2048 * 2 * 3), (99, 4, 416, 1)),
    ((12576, 512, 64, 64, 64 * 512 * 4), (197, 8, 1600, 8)),              # fp32 operands: bn * K * 4
    ((12576, 512, 128, 64, 64 * 4096 * 4), (99, 8, 832, 2)),
    ((4097, 130, 64, 64, 64 * 8192 * 4), (65, 3, 216, 1)),                # a panel of the whole 2 MB: one column per group
    ((3968, 512, 128, 128, 128 * 512 * 4), (31, 4, 124, 0)),              # 31 row tiles: plain order
    ((12576, 128, 128, 128, 128 * 512 * 4), (99, 1, 99, 0)),              # one column tile: plain order
]


@pytest.mark.parametrize("args, expect", TILE_GRID)
def test_tile_grid(handle, args, expect):
    out = (ctypes.c_int * 4)()
    handle.mt_debug_tile_grid(*args, out)
    assert tuple(out) == expect


# (K, tiles, split_k, automatic target, K rounding, form) -> (k_chunk, ranges, grid_y)
SPLIT_K = [
    # K-range-major without the cap (the plane loop): always, also for the caller's own split_k
    ((12576, 48, 0, 640, 16, XCD), (800, 16, 16)),
    ((12576, 128, 0, 640, 16, XCD), (1584, 8, 8)),
    ((12576, 16, 0, 640, 16, XCD), (320, 40, 40)),
    ((2047, 16, 0, 640, 16, XCD), (256, 8, 8)),
    ((100, 16, 0, 640, 16, XCD), (16, 7, 8)),                             # 7 non-empty ranges in a group of 8
    ((12576, 48, 3, 640, 16, XCD), (1584, 8, 8)),
    ((12576, 48, 20, 640, 16, XCD), (528, 24, 24)),
    # K-range-major with the cap (the split loop's weight gradients, K >= 2048)
    ((2048, 16, 0, 640, 16, XCD_CAPPED), (256, 8, 8)),
    ((4000, 16, 0, 640, 16, XCD_CAPPED), (512, 8, 8)),
    ((12576, 48, 0, 640, 16, XCD_CAPPED), (800, 16, 16)),
    # plain
    ((2047, 16, 0, 640, 16, PLAIN), (304, 7, 7)),
    ((4128, 16, 5, 640, 16, PLAIN), (832, 5, 5)),
    ((640, 16, 3, 640, 16, PLAIN), (224, 3, 3)),
    ((12576, 16, 0, 2048, 16, PLAIN), (272, 47, 47)),
    ((12576, 16, 0, 2048, 32, PLAIN), (288, 44, 44)),                     # the LDS-DMA loop's BK = 32 variants
    ((4128, 6, 0, 2048, 16, PLAIN), (272, 16, 16)),
    ((512 * 147 * 147, 1, 0, 2048, 16, PLAIN), (5408, 2046, 2046)),
    ((640, 16, 0, 0, 16, PLAIN), (640, 1, 1)),                            # no automatic target: split_k <= 0 means 1
]


@pytest.mark.parametrize("args, expect", SPLIT_K)
def test_split_k_ranges(handle, args, expect):
    out = (ctypes.c_int * 4)()
    handle.mt_debug_split_k(*args, out)
    assert tuple(out)[:3] == expect
    assert out[3] == (args[5] != PLAIN)                                   # xcd_k
