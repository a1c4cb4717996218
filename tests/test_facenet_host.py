"""Host side of the FaceNet InceptionResnetV1 embedder: module, restatement (tests/facenet_ref.py) and the hand-written manifest
(tests/golden/facenet_inception_resnet_v1_manifest.json) agree on every key and shape; state dicts round-trip; the stage sizes of
the engine equal the restatement's; the BatchNorm fold equals conv + BN in fp64; the refusals raise before the library is touched.
No device is touched."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import mintime_amd
from mintime_amd import facenet as FN
from mintime_amd import facenet_engine as E
from mintime_amd import lib as L
from tests import facenet_ref as R
from tests.util import GOLDEN, declared_params, header_text


@pytest.fixture(scope="module")
def net():
    return mintime_amd.InceptionResnetV1()


def _manifest():
    with open(os.path.join(GOLDEN, "facenet_inception_resnet_v1_manifest.json")) as fh:
        return json.load(fh)


def test_module_restatement_and_manifest_agree(net):
    man, sd = _manifest(), net.state_dict()
    assert len(man) == len(sd) == 714
    assert man == R.manifest()
    assert {k: list(v.shape) for k, v in sd.items()} == man
    assert sum(p.numel() for p in net.parameters()) == 23482624
    assert sum(isinstance(m, torch.nn.Conv2d) for m in net.modules()) == 132
    with_logits = mintime_amd.InceptionResnetV1(num_classes=8631).state_dict()
    assert len(with_logits) == 716 and set(with_logits) - set(sd) == {"logits.weight", "logits.bias"}
    assert {k: list(v.shape) for k, v in with_logits.items()} == R.manifest(8631)
    bn = net.conv2d_1a.bn
    assert (bn.eps, bn.momentum, net.last_bn.eps) == (1e-3, 0.1, 1e-3) and net.conv2d_1a.conv.bias is None
    assert net.repeat_1[0].conv2d.bias is not None and net.block8.noReLU and not net.repeat_3[4].noReLU
    assert (net.repeat_1[0].scale, net.repeat_2[0].scale, net.repeat_3[0].scale, net.block8.scale) == (0.17, 0.10, 0.20, 1.0)


def test_package_surface_and_entry_points():
    assert mintime_amd.InceptionResnetV1 is FN.InceptionResnetV1 and "InceptionResnetV1" in mintime_amd.__all__
    assert mintime_amd.fixed_image_standardization is FN.fixed_image_standardization
    x = torch.tensor([0.0, 127.5, 255.0])
    assert torch.equal(mintime_amd.fixed_image_standardization(x), torch.tensor([-127.5 / 128, 0.0, 127.5 / 128]))
    assert "UNCHECKED" in FN.__doc__
    handle = ctypes.CDLL(L.LIB_PATH)
    for name, count in (("mt_conv2d_fwd", 7), ("mt_face_ingest", 12), ("mt_maxpool2d_fwd", 12), ("mt_avgpool_rows", 8),
                        ("mt_l2_normalize_rows", 8)):
        params = declared_params(name)
        assert params[-1] == "void* stream"
        assert name in L.PROTOTYPES and len(L.PROTOTYPES[name]) == len(params) == count
        assert hasattr(handle, name) and hasattr(handle, "mti_" + name[3:])
    assert "mt_conv2d_desc" in header_text() and os.path.exists(os.path.join(L.CSRC, "facenet.hip"))
    thunks = open(os.path.join(L.CSRC, "plan_thunks.inc")).read()
    body = thunks[thunks.index('extern "C" int mt_conv2d_fwd('):]
    assert "const auto d_v = *d;" in body[:body.index("return rc;")]           # the descriptor is copied into the recorded call
    assert ctypes.sizeof(L.Conv2dDesc) == 14 * 4 + 4 + 4 + 3 * 8                 # 14 ints, a float, padding, 3 pitches


def test_state_dict_round_trips_with_prefix_and_logits():
    sd = R.seeded_state(3)
    a = mintime_amd.InceptionResnetV1()
    a.load_state_dict({"module." + k: v for k, v in sd.items()})
    got = a.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    full = dict(sd)
    full["logits.weight"], full["logits.bias"] = torch.randn(8631, 512), torch.randn(8631)
    with pytest.raises(RuntimeError):
        a.load_state_dict(full)                                                  # no home for logits.*
    b = mintime_amd.InceptionResnetV1(num_classes=8631)
    b.load_state_dict(full)
    assert torch.equal(b.state_dict()["logits.bias"], full["logits.bias"])


def test_weights_path_loads_a_local_state_dict(tmp_path):
    sd = R.seeded_state(4)
    sd["logits.weight"], sd["logits.bias"] = torch.zeros(10575, 512), torch.zeros(10575)
    path = str(tmp_path / "casia.pt")
    torch.save(sd, path)
    m = mintime_amd.InceptionResnetV1(pretrained="casia-webface", weights_path=path)
    assert m.num_classes == 10575 and torch.equal(m.state_dict()["block8.conv2d.weight"], sd["block8.conv2d.weight"])


def test_stage_sizes_equal_the_restatements(net):
    for n in range(75, 201):
        assert E.stage_sizes(n) == R.stage_sizes(n)
        assert E.stage_sizes(n)[-1] >= 1
    assert E.stage_sizes(75)[-1] == 1 and E.stage_sizes(128) == [63, 61, 61, 30, 30, 28, 13, 6, 2]
    with pytest.raises(ValueError):
        R.stage_sizes(74)
    with pytest.raises(ValueError):
        E.check_side(74, 128)
    with pytest.raises(ValueError):
        E.check_side(128, 74)
    E.check_side(75, 76)
    # the launch list itself ends on the same grid and counts the network's multiply-adds
    b = E._Builder(net.engine(), 1, 80, 128)
    last = E._program(b, net)
    convs = [op[1] for op in b.ops if op[0] == "conv"]
    assert (last.C, last.h, last.w) == (512, 1, 1) and len(convs) == 110
    assert convs[-2].Ho == R.stage_sizes(80)[-1] and convs[-2].Wo == R.stage_sizes(128)[-1]
    b = E._Builder(net.engine(), 1, 128, 128)
    E._program(b, net)
    macs = sum(d.Ho * d.Wo * d.K * d.kh * d.kw * (3 if d.C == 4 else d.C) for d in (op[1] for op in b.ops if op[0] == "conv"))
    assert abs(macs - 512 * 1792 - 811.4e6) < 0.05e6


def test_host_fold_equals_conv_plus_bn_in_fp64():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(8, 4, 3, 3, generator=g, dtype=torch.float64)
    gamma, beta = 0.5 + torch.rand(8, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    mean, var = torch.randn(8, generator=g, dtype=torch.float64), 0.5 + torch.rand(8, generator=g, dtype=torch.float64)
    x = torch.randn(2, 4, 6, 5, generator=g, dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, w, None, 1, 1), mean, var, gamma, beta, False, 0.1, 1e-3)
    wf, bf = E.fold_conv_bn(w, gamma, beta, mean, var)
    got = F.conv2d(x, wf, bf, 1, 1)
    assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()
    packed = E.pack_weight(wf)
    assert packed.shape == (8, 3, 3, 4) and torch.equal(packed[3, 1, 2], wf[3, :, 1, 2])
    assert E.pack_weight(torch.ones(2, 3, 3, 3)).shape == (2, 3, 3, 4) and (E.pack_weight(torch.ones(2, 3, 3, 3))[..., 3] == 0).all()
    lw = torch.randn(8, 16, generator=g, dtype=torch.float64)                     # last_linear + last_bn
    xl = torch.randn(3, 16, generator=g, dtype=torch.float64)
    wf, bf = E.fold_conv_bn(lw, gamma, beta, mean, var)
    want = F.batch_norm(F.linear(xl, lw), mean, var, gamma, beta, False, 0.1, 1e-3)
    assert (F.linear(xl, wf, bf) - want).abs().max().item() <= 1e-13 * want.abs().max().item()


def test_refusals(net):
    with pytest.raises(NotImplementedError):
        mintime_amd.InceptionResnetV1(classify=True)
    for name in ("vggface2", "casia-webface"):
        with pytest.raises(RuntimeError, match="weights_path"):
            mintime_amd.InceptionResnetV1(pretrained=name)
    m = mintime_amd.InceptionResnetV1()
    assert m.training
    with pytest.raises(NotImplementedError, match="inference only"):
        m(torch.zeros(1, 3, 80, 80))
    m.eval()
    with pytest.raises(L.MintimeHipError, match="no CPU path"):
        m(torch.zeros(1, 3, 80, 80))
    with pytest.raises(L.MintimeHipError, match="no CPU path"):
        m.embed_crops(torch.zeros(1, 80, 80, 3, dtype=torch.uint8))
    with pytest.raises(L.MintimeHipError):
        m.conv2d_1a(torch.zeros(1, 3, 80, 80))
    assert not os.path.isdir(os.path.join(os.path.dirname(L.CSRC), "..", "facenet_pytorch"))     # the real package is not shadowed
