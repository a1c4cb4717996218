"""Host side of the input-crop gradient: the two stem data-gradient entry points are declared and bound, the ABI number did not move
(added entry points are backward compatible), and harness.input_gradient refuses what has no gradient before touching a device."""
import re

import pytest
import torch

import mintime_amd
from mintime_amd import harness
from mintime_amd import lib as L
from tests.util import declared_params, header_text

SYMBOLS = ("mt_stem_conv_dgrad", "mt_stem_conv_dgrad_valid")


@pytest.mark.parametrize("name", SYMBOLS)
def test_entry_point_is_declared_and_bound(name):
    params = declared_params(name)
    assert params[-1] == "void* stream"                          # a launching entry point: csrc/gen_plan.py gives it a recording thunk
    assert name in L.PROTOTYPES and len(L.PROTOTYPES[name]) == len(params) == 9


def test_abi_version_did_not_move():
    assert L.ABI_VERSION == 123 and int(re.search(r"#define\s+MT_VERSION\s+(\d+)", header_text()).group(1)) == 123


class _NeverCalled(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("input_gradient ran a module before checking its input")


def test_input_gradient_refuses_uint8_and_host_tensors():
    ex, model = _NeverCalled(), _NeverCalled()
    labels = torch.zeros(1)
    with pytest.raises(ValueError, match="floating-point"):
        harness.input_gradient(ex, model, dict(videos=torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8), labels=labels))
    with pytest.raises(ValueError, match="on the device"):
        harness.input_gradient(ex, model, dict(videos=torch.zeros(1, 2, 8, 8, 3), labels=labels))
