"""Host side of SlowFast's input-clip gradient: the inverse frame map of the ingest's adjoint, the two new entry points' declarations
and bindings, and the refusals of harness.slowfast_input_gradient / harness.input_gradient before anything touches a device."""

import pytest
import torch

import mintime_amd
from mintime_amd import harness
from mintime_amd import lib as L
from mintime_amd import slowfast as S
from tests.util import declared_params

frame_sources = S.frame_sources             # the module needs the feature: without it nothing here is collected


def _check_sources(fidx, F):
    start, js = S.frame_sources(fidx, F)
    assert len(start) == F + 1 and start[0] == 0 and start[-1] == len(fidx)
    assert sorted(js) == list(range(len(fidx)))                  # every output frame exactly once
    for f in range(F):
        seg = js[start[f]:start[f + 1]]
        assert seg == [j for j, g in enumerate(fidx) if g == f]  # the frame's selectors, ascending; empty when nobody selected it


@pytest.mark.parametrize("F", range(1, 71))
def test_frame_sources_inverts_uniform_temporal_subsample(F):
    fidx = torch.linspace(0, F - 1, 32).long().tolist()
    assert fidx == S.frame_indices(F, 32)
    _check_sources(fidx, F)
    start, _ = S.frame_sources(fidx, F)
    if F > 32:
        assert any(start[f] == start[f + 1] for f in range(F))   # skipped frames have empty ranges


def test_frame_sources_of_the_slow_selection_and_of_both_pathways():
    si = torch.linspace(0, 31, 8).long().tolist()
    _check_sources(si, 32)
    start, js = S.frame_sources(si, 32)
    assert sum(start[f + 1] - start[f] == 0 for f in range(32)) == 24
    # the transform's one launch: slow frames first, then the fast ones, of a 40-frame clip
    fi = S.frame_indices(40, 32)
    _check_sources([fi[j] for j in si] + fi, 40)
    with pytest.raises(ValueError):
        S.frame_sources([0, 5], 5)


@pytest.mark.parametrize("name,nparams", [("mt_sf_stem_dgrad", 11), ("mt_sf_ingest_bwd", 18)])
def test_entry_point_is_declared_and_bound(name, nparams):
    params = declared_params(name)
    assert params[-1] == "void* stream"                          # a launching entry point: csrc/gen_plan.py gives it a recording thunk
    assert name in L.PROTOTYPES and len(L.PROTOTYPES[name]) == len(params) == nparams
    assert L.ABI_VERSION == 123                                  # added entry points do not move the ABI number


class _NeverCalled(S.SlowFast):
    def __init__(self):
        torch.nn.Module.__init__(self)

    def forward(self, *a, **k):
        raise AssertionError("slowfast_input_gradient ran the model before checking its input")


def test_slowfast_input_gradient_refuses_uint8_and_host_tensors():
    model = _NeverCalled()
    labels = torch.zeros(1)
    u8 = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="floating-point"):
        harness.slowfast_input_gradient(model, u8, labels)
    with pytest.raises(ValueError, match="on the device"):
        harness.slowfast_input_gradient(model, u8.float(), labels)
    # harness.input_gradient dispatches a SlowFast model there (no extractor)
    with pytest.raises(ValueError, match="floating-point"):
        harness.input_gradient(None, model, dict(videos=u8, labels=labels))
    with pytest.raises(ValueError, match="on the device"):
        harness.input_gradient(None, model, dict(videos=u8.float(), labels=labels))


def test_input_gradient_still_refuses_an_unknown_model_type():
    class Other(torch.nn.Module):
        pass

    class OnDevice(torch.Tensor):            # passes the "on the device" check without a device; the type check comes next
        is_cuda = True
    videos = torch.zeros(1, 2, 8, 8, 3).as_subclass(OnDevice)
    with pytest.raises(TypeError, match="Other"):
        harness.input_gradient(None, Other(), dict(videos=videos, labels=torch.zeros(1)))
