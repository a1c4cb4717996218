"""CPU tests of the Baseline model (reference models/baseline.py, `--model 0`): the import path the reference scripts use, state-dict
compatibility with the reference, and the argument checks (no compute calls without a GPU)."""
import importlib
import json

import pytest
import torch

import mintime_amd
from mintime_amd import arch, lib, synth
from tests.util import golden

# every model import the reference scripts make at module level (file:line, module, name): with this repository's root on PYTHONPATH
# ahead of the reference they must all resolve through this repository's `models/` package
REFERENCE_MODEL_IMPORTS = [
    ("train.py:27", "models.size_invariant_timesformer", "SizeInvariantTimeSformer"),
    ("train.py:28", "models.efficientnet.efficientnet_pytorch", "EfficientNet"),
    ("train.py:32", "models.baseline", "Baseline"),
    ("train.py:33", "models.xception", "xception"),
    ("test.py:29", "models.size_invariant_timesformer", "SizeInvariantTimeSformer"),
    ("test.py:30", "models.efficientnet.efficientnet_pytorch", "EfficientNet"),
    ("test.py:34", "models.baseline", "Baseline"),
    ("test.py:35", "models.xception", "xception"),
    ("predict.py:24", "models.size_invariant_timesformer", "SizeInvariantTimeSformer"),
    ("predict.py:25", "models.efficientnet.efficientnet_pytorch", "EfficientNet"),
    ("predict.py:26", "models.baseline", "Baseline"),
    ("predict.py:30", "models.xception", "xception"),
]


def test_models_baseline_resolves_to_the_package_class():
    from models.baseline import Baseline
    assert Baseline is mintime_amd.Baseline
    assert Baseline.__module__.endswith(".baseline")


@pytest.mark.parametrize("where,module,name", REFERENCE_MODEL_IMPORTS, ids=[w for w, _, _ in REFERENCE_MODEL_IMPORTS])
def test_reference_scripts_model_imports_resolve_here(where, module, name):
    mod = importlib.import_module(module)
    assert hasattr(mod, name), f"{where}: `from {module} import {name}` fails"
    obj = getattr(mod, name)
    assert getattr(obj, "__module__", "").startswith(mintime_amd.__name__), (where, obj)


def test_state_dict_keys_and_shapes_equal_the_reference():
    g = golden("baseline_head")
    ref_keys = [str(k) for k in g["state_keys"]]
    ref_shapes = json.loads(str(g["state_shapes"]))
    cfg = arch.default_baseline_config(int(g["channels"]), int(g["frames"]))
    sd = mintime_amd.Baseline(cfg).state_dict()
    assert list(sd) == ref_keys
    assert [list(v.shape) for v in sd.values()] == ref_shapes


@pytest.mark.parametrize("prefix", ["", "module."])
def test_reference_shaped_state_dict_loads_strictly(prefix):
    """Checkpoints of train.py (saved bare or through nn.DataParallel: `module.` keys) load into the module and its wrapper."""
    cfg = arch.default_baseline_config(1280, 16)
    sd = synth.baseline_state(cfg, 3)
    model = mintime_amd.Baseline(cfg)
    target = torch.nn.DataParallel(model) if prefix else model          # DataParallel on a CPU-only host: a plain wrapper
    target.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    back = target.state_dict()
    assert sorted(back) == sorted(prefix + k for k in sd)


def test_default_init_matches_nn_linear_bounds():
    cfg = arch.default_baseline_config(1280, 16)
    torch.manual_seed(0)
    sd = mintime_amd.Baseline(cfg).state_dict()
    for key, fan_in in (("mlp_head.0", 1280), ("mlp_head.1", 512)):
        bound = 1.0 / fan_in ** 0.5
        for t in (sd[key + ".weight"], sd[key + ".bias"]):
            assert float(t.abs().max()) <= bound
            if t.numel() > 1:
                assert float(t.std()) > 0.3 * bound


def test_num_classes_other_than_one_is_refused():
    cfg = arch.default_baseline_config(1280, 16)
    cfg["model"]["num-classes"] = 2
    with pytest.raises(NotImplementedError, match="rank-1"):
        mintime_amd.Baseline(cfg)


def test_cpu_input_raises():
    model = mintime_amd.Baseline(arch.default_baseline_config(1280, 16))
    with pytest.raises(lib.MintimeHipError):
        model(torch.zeros(2, 1280, 7, 7))
