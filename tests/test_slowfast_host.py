"""SlowFast R50 (`--model 2`) host-side surface: imports, the state-dict contract, checkpoints, the head swap, the ingest index rules.
tests/golden/slowfast_r50_manifest.json is a HAND-WRITTEN manifest of pytorchvideo slowfast_r50's keys and shapes, written from the
published structure; it has not been checked against the pytorchvideo package itself."""
import json
import os

import pytest
import torch

from .util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _manifest():
    with open(os.path.join(GOLDEN, "slowfast_r50_manifest.json")) as f:
        return json.load(f)["keys"]


def test_models_slowfast_and_hubconf_import():
    from models.slowfast import SlowFast, slowfast_r50
    import hubconf
    assert hubconf.slowfast_r50 is slowfast_r50
    assert isinstance(slowfast_r50(), SlowFast)


def test_torch_hub_local_load():
    m = torch.hub.load(ROOT, "slowfast_r50", source="local")
    assert type(m).__name__ == "SlowFast"


def test_state_dict_matches_manifest():
    from models.slowfast import slowfast_r50
    sd = slowfast_r50().state_dict()
    man = _manifest()
    assert list(sd) == list(man)
    assert {k: list(v.shape) for k, v in sd.items()} == man


def test_module_prefixed_checkpoint_loads(tmp_path):
    from models.slowfast import slowfast_r50
    src = slowfast_r50()
    sd = {"module." + k: v.clone() for k, v in src.state_dict().items()}
    path = tmp_path / "ckpt.pth"
    torch.save(sd, path)
    m = slowfast_r50(weights_path=str(path))
    for k, v in m.state_dict().items():
        assert torch.equal(v, src.state_dict()[k]), k
    m2 = slowfast_r50()
    m2.load_state_dict(sd)
    assert torch.equal(m2.blocks[6].proj.weight, src.blocks[6].proj.weight)


def test_proj_can_be_replaced():
    from models.slowfast import slowfast_r50
    m = slowfast_r50()
    m.blocks[6].proj = torch.nn.Linear(2304, 1)
    sd = m.state_dict()
    assert tuple(sd["blocks.6.proj.weight"].shape) == (1, 2304) and tuple(sd["blocks.6.proj.bias"].shape) == (1,)
    names = [n for n, _ in m.named_parameters()]
    assert names[-2:] == ["blocks.6.proj.weight", "blocks.6.proj.bias"]


@pytest.mark.parametrize("F", [8, 16, 32])
def test_ingest_index_rules(F):
    import mintime_amd
    fi = mintime_amd.slowfast.frame_indices(F, 32)
    assert fi == torch.linspace(0, F - 1, 32).long().tolist()
    si = mintime_amd.slowfast.frame_indices(32, 8)
    assert si == torch.linspace(0, 31, 8).long().tolist()


def test_pretrained_without_path_fails_cleanly():
    from models.slowfast import slowfast_r50
    with pytest.raises(RuntimeError, match="network access"):
        slowfast_r50(pretrained=True)


def test_init_matches_pytorchvideo_resnet_style():
    from models.slowfast import slowfast_r50
    m = slowfast_r50()
    sd = m.state_dict()
    assert torch.all(sd["blocks.1.multipathway_blocks.0.res_blocks.0.branch2.norm_c.weight"] == 0)
    assert torch.all(sd["blocks.1.multipathway_blocks.0.res_blocks.0.branch2.norm_a.weight"] == 1)
    assert m.blocks[6].dropout.p == 0.5


def test_transform_refuses_other_sizes():
    import mintime_amd
    with pytest.raises(NotImplementedError):
        mintime_amd.slowfast_input_transform(torch.zeros(1, 8, 128, 128, 3, dtype=torch.uint8))
