"""Host side of the SlowFast input transform's ShortSideScale + CenterCropVideo (interpolation="bilinear"): the size and crop rules,
the per-axis tap tables and their inverse, the refusals that need no device, and the two entry points' declarations and bindings."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mintime_amd
from mintime_amd import lib as L
from mintime_amd import slowfast as S

from . import sf_resize_ref as RR
from .util import declared_params

# (H, W, side, crop) -> (Hr, Wr), (top, left)
GEOMETRY = [
    ((20, 28, 16, 16), (16, 22), (0, 3)),
    ((28, 20, 16, 16), (22, 16), (3, 0)),
    ((9, 13, 16, 16), (16, 23), (0, 4)),            # upscale
    ((16, 21, 16, 16), (16, 21), (0, 2)),           # 2.5 rounds to even, down
    ((16, 23, 16, 16), (16, 23), (0, 4)),           # 3.5 rounds to even, up
    ((37, 53, 24, 16), (24, 34), (4, 9)),
    ((13, 9, 16, 12), (23, 16), (6, 2)),
]
IDS = ["x".join(map(str, g[0])) for g in GEOMETRY]


@pytest.mark.parametrize("case,size,corner", GEOMETRY, ids=IDS)
def test_resize_geometry(case, size, corner):
    assert S.resize_geometry(*case) == size + corner
    assert RR.short_side_size(*case[:3]) == size                 # the tests' own restatement agrees


@pytest.mark.parametrize("case,size,corner", GEOMETRY, ids=IDS)
def test_tap_tables_reproduce_interpolate_in_fp64(case, size, corner):
    H, W, side, crop = case
    (Hr, Wr), (top, left) = size, corner
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randint(0, 256, (2, 3, H, W), generator=g).double()
    want = F.interpolate(x, size=(Hr, Wr), mode="bilinear", align_corners=False)[..., top:top + crop, left:left + crop].numpy()
    h0, h1, hl = [t.numpy() for t in S.axis_taps(H, Hr, top, crop, dtype=torch.float64)]
    w0, w1, wl = [t.numpy() for t in S.axis_taps(W, Wr, left, crop, dtype=torch.float64)]
    assert hl.dtype == np.float64 and h0.dtype == np.int32
    xn = x.numpy()
    rows = (1 - hl)[:, None] * xn[:, :, h0, :] + hl[:, None] * xn[:, :, h1, :]
    got = (1 - wl) * rows[..., w0] + wl * rows[..., w1]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-11
    # the fp32 tables the kernels read pick indices inside the frame and weights in [0, 1]
    for n_in, n_out, first in ((H, Hr, top), (W, Wr, left)):
        i0, i1, lam = S.axis_taps(n_in, n_out, first, crop)
        assert lam.dtype == torch.float32 and i0.dtype == i1.dtype == torch.int32
        assert 0 <= int(i0.min()) and int(i1.max()) <= n_in - 1 and bool(((i1 == i0) | (i1 == i0 + 1)).all())
        assert float(lam.min()) >= 0 and float(lam.max()) <= 1


@pytest.mark.parametrize("case,size,corner", GEOMETRY, ids=IDS)
def test_axis_sources_inverts_the_taps(case, size, corner):
    """Scattering every output index's two weights onto its taps gives the same matrix as the CSR lists, in ascending output order."""
    H, W, side, crop = case
    for n_in, n_out, first in ((H, size[0], corner[0]), (W, size[1], corner[1])):
        i0, i1, lam = S.axis_taps(n_in, n_out, first, crop)
        start, out, wt = S.axis_sources(i0, i1, lam, n_in)
        assert len(start) == n_in + 1 and start[0] == 0 and start[-1] == len(out) == len(wt)
        want = torch.zeros(n_in, crop, dtype=torch.float64)
        for d in range(crop):
            want[int(i0[d]), d] += float(1 - lam[d])
            want[int(i1[d]), d] += float(lam[d])
        got = torch.zeros(n_in, crop, dtype=torch.float64)
        for s in range(n_in):
            seg = out[start[s]:start[s + 1]]
            assert seg == sorted(seg)
            for d, w in zip(seg, wt[start[s]:start[s + 1]]):
                assert w != 0
                got[s, d] += w
        assert torch.equal(got, want)
        assert torch.allclose(got.sum(0), torch.ones(crop, dtype=torch.float64), atol=1e-6)      # each output's weights add to 1


def test_crop_larger_than_the_resized_frame_raises():
    with pytest.raises(ValueError, match="no smaller than crop_size"):
        S.resize_geometry(20, 28, 16, 17)
    # the transform refuses before it needs a device
    with pytest.raises(ValueError, match="no smaller than crop_size"):
        mintime_amd.slowfast_input_transform(torch.zeros(1, 8, 20, 28, 3, dtype=torch.uint8), crop_size=24, side_size=16,
                                             interpolation="bilinear")
    with pytest.raises(ValueError, match="no smaller than crop_size"):
        S.ingest_resize(torch.zeros(1, 8, 20, 28, 3), [0], True, "bfhwc", (16, 22, 0, 0, 16, 23))


def test_unknown_interpolation_raises():
    v = torch.zeros(1, 8, 20, 28, 3, dtype=torch.uint8)
    for mode in ("nearest", "bicubic", "BILINEAR", ""):
        with pytest.raises(NotImplementedError, match="bilinear"):
            mintime_amd.slowfast_input_transform(v, crop_size=16, side_size=16, interpolation=mode)
    with pytest.raises(NotImplementedError, match="bilinear"):                # also where no resize would be needed
        mintime_amd.slowfast_input_transform(torch.zeros(1, 8, 16, 16, 3, dtype=torch.uint8), crop_size=16, side_size=16,
                                             interpolation="nearest")


def test_the_default_still_refuses_other_sizes():
    for v, kw in ((torch.zeros(1, 8, 128, 128, 3, dtype=torch.uint8), {}),
                  (torch.zeros(1, 8, 20, 28, 3, dtype=torch.uint8), dict(crop_size=16, side_size=16)),
                  (torch.zeros(1, 3, 8, 20, 28), dict(crop_size=16, side_size=16, interpolation=None)),
                  (torch.zeros(1, 8, 16, 16, 3), dict(crop_size=12, side_size=16))):
        with pytest.raises(NotImplementedError, match="interpolation"):
            mintime_amd.slowfast_input_transform(v, **kw)


@pytest.mark.parametrize("name,nparams", [("mt_sf_ingest_resize", 27), ("mt_sf_ingest_resize_bwd", 30)])
def test_entry_point_is_declared_and_bound(name, nparams):
    params = declared_params(name)
    assert params[-1] == "void* stream"                          # a launching entry point: csrc/gen_plan.py gives it a recording thunk
    assert name in L.PROTOTYPES and len(L.PROTOTYPES[name]) == len(params) == nparams
    assert os.path.exists(os.path.join(L.CSRC, "sf_resize.hip"))
